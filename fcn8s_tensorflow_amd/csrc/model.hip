// Host side of libfcn8s_hip.so: the model handle (variables, HBM arena,
// optimizer slots, metric accumulators) and the launch sequences that replace
// the reference's three hot sess.run sites (fcn8s_tensorflow.py:554-572,
// 685-689, 764-770).  Everything is enqueued on one HIP stream; the only host
// synchronisations are the ones the reference's fetches imply (loss, metrics,
// predictions).
#include "../../include/fcn8s_hip.h"
#include "fcn8s_internal.h"
#include "device_buffer.h"
#include "pass_state.h"
#include "conv_route.h"
#include <cstdarg>
#include <functional>

#include <dlfcn.h>
#include <atomic>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <mutex>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace fcn8s;

// The few RCCL (= NCCL API) types behind the entry points this file resolves with dlsym: declared here, with the values of rccl.h (RCCL 2.x; the
// NCCL API keeps them stable), so that building the library needs no RCCL development headers -- a single-GPU user never touches RCCL at all.
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0, ncclUnhandledCudaError = 1, ncclSystemError = 2, ncclInternalError = 3, ncclInvalidArgument = 4, ncclInvalidUsage = 5,
               ncclRemoteError = 6, ncclInProgress = 7 } ncclResult_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
typedef enum { ncclFloat = 7, ncclDouble = 8 } ncclDataType_t;
}
static_assert(sizeof(ncclUniqueId) == FCN8S_COMM_ID_BYTES, "fcn8s_comm_unique_id hands out ncclUniqueId bytes");

namespace {

thread_local std::string g_last_error;
thread_local int t_deferred_code = 0;
thread_local std::string t_deferred_text;

struct ParamInfo {
    std::string name;
    int ndim;
    int64_t shape[4];
    size_t offset, numel;
};

struct ProfGroup {
    std::string name;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;          // owned
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_shared;   // borrowed from another group (per-kernel-symbol view)
    double flops = 0, bytes = 0;
    int64_t launches = 0;
};

struct Act { float* p = nullptr; size_t n = 0; int H = 0, W = 0, C = 0; };

const int kConvsPerBlock[5] = {2, 2, 3, 3, 3};

// One weighted layer of the encoder -- conv1_1 .. conv5_3, fc6, fc7, in forward order -- as the current plan sees it (fcn8s_model::layers): filled
// by plan_workspace, its arena views resolved by carve_workspace.  forward(), backward_blocks() and the read-back entry points walk these entries;
// only the plan spells a layer's name.  The per-pass ledger (pass_state.h) stays keyed by `name`.
// INVARIANT: the route facts are functions of the model's widths, the planned (N, H, W) and RouteOpts (conv_route.h), and the table lives exactly as
// long as the arena it was planned with: every option RouteOpts reads -- winograd_min_cin, winograd_tile, winograd_tile_hires,
// winograd_hires_pixels, winograd_fc6 -- drops the arena in fcn8s_set_option, fcn8s_set_precision drops it when a direct mode takes the first and
// the last over, wino_force_tile belongs to the bare op models alone, and no pass starts without ensure_workspace.  Options that pick a kernel per
// launch without dropping the arena (conv1_in_transform, ...; bf16_train's Bf16Opts) and what only a pass knows (train, the precision branch) are never
// stored here: the call sites AND them with the stored fact, and ask the bf16_train rules in every pass.
struct Layer {
    char name[8], pool_name[8], pool_in[12];     // "conv3_2" / "fc6"; the last conv of a block: "pool3" and the key of its pool's bf16 / e4m3 input copy, "pool3in"
    int block, pos, nconv;                       // 1-based VGG block, position in it, convs in it (fc6, fc7: blocks 6, 7 of one layer each)
    int h, w, cin, cout, K, real_cin;            // map, channels as the kernels see them (conv1_1: cin 4, real_cin 3), kernel size
    int prev, next;                              // the entries before / behind it, -1 at the ends (in_block_prev / in_block_next: on the same map)
    size_t w_off, b_off;                         // kernel and bias: floats from the start of the parameter buffer (the same in d_grads and d_wt)
    int i_y, i_rb, i_wv, i_pool, i_pidx;         // the plan's items (-1: none); carve_workspace makes the views below from them
    float *y, *wv, *pool; unsigned* rb; unsigned char* pidx;      // activation, kept V, ReLU bit record; the block's pool and argmax bytes (every conv of the block points at them)
    // route facts (conv_route.h), each named after its rule: the ones a pass reads outside conv_fwd / conv_wgrad / conv_dgrad, which ask the rules themselves
    // (wv != nullptr: keeps_v)
    int tile;                                    // wino_tile_for on this map
    RbWriter rb_writer;
    bool out_in_next, conv1_in_next;             // (this layer and its in-block successor)
    bool dm_from_next, pool_in_transform, gemm_out_fused64;
    ConvShape shape(int N) const { return ConvShape{N, h, w, cin, cout, K}; }
    bool first() const { return real_cin != 0; }
    bool last_of_block() const { return pos == nconv; }
};

}  // namespace

namespace fcn8s {
void defer_error(int code, const char* fmt, ...)
{
    if (t_deferred_code) return;
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    t_deferred_code = code; t_deferred_text = buf;
}
int take_deferred_error(std::string* text)
{
    const int c = t_deferred_code;
    if (c && text) *text = t_deferred_text;
    t_deferred_code = 0; t_deferred_text.clear();
    return c;
}
}  // namespace fcn8s

// FCN8S_PREC_FP8_INFER: a layer's padded e4m3 input copy (64-channel planes ps bytes apart; the border is zeroed whenever the geometry changes) with the
// exponent its codes carry, and a layer's quantized weight bank (planes [K K Cin / 64][Cout][64], per-column exponents, the amax scratch behind them)
struct Q8Buf { DeviceBuf<unsigned char> p; int N = 0, H = 0, W = 0, C = 0, pad = -1, ex = 0; long long ps = 0; };
struct W8Bank { DeviceBuf<unsigned char> wq; int* ew = nullptr; unsigned* amax = nullptr; };      // (ew, amax: views into wq)

struct fcn8s_model {
    int C = 20, fc6k = 7, device = 0;
    int widths[7] = {64, 128, 256, 512, 512, 4096, 4096};
    uint64_t seed = 0;
    std::vector<ParamInfo> params;
    std::map<std::string, int> index;
    size_t total = 0;
    size_t bucket_off[FCN8S_MAX_BUCKETS] = {0}, bucket_n[FCN8S_MAX_BUCKETS] = {0};
    hipEvent_t bucket_ev[FCN8S_MAX_BUCKETS] = {nullptr};                 // recorded right behind the last kernel that writes into the bucket
    bool bucket_final[FCN8S_MAX_BUCKETS] = {false};                      // ... this backward pass (fcn8s_bucket_wait)
    // the library's own RCCL communicator (fcn8s_comm_*): one rank per model, collectives on a stream of its own behind the bucket events
    ncclComm_t comm = nullptr; int comm_rank = 0, comm_world = 1;
    hipStream_t comm_stream = nullptr;
    // slot b < FCN8S_MAX_BUCKETS: the all-reduce of gradient bucket b; slot FCN8S_MAX_BUCKETS: the parameter broadcast / the metrics all-reduce
    static constexpr int kCommSlots = FCN8S_MAX_BUCKETS + 1, kCommMisc = FCN8S_MAX_BUCKETS;
    hipEvent_t comm_done[kCommSlots] = {nullptr}; bool comm_pending[FCN8S_MAX_BUCKETS] = {false};
    // ... and its watchdog (world > 1): a thread that polls ncclCommGetAsyncError and the age of every all-reduce still in flight; on an
    // asynchronous error or after comm_timeout_ms it calls ncclCommAbort (RCCL's kernels then leave the streams they block) and records
    // why -- every later fcn8s_comm_* / fcn8s_apply_update call returns FCN8S_ERR_RCCL with that text instead of waiting for a dead peer
    std::mutex comm_mu;                                                   // guards comm (enqueue vs. abort), comm_enq_ns, comm_error
    std::thread comm_watch; std::atomic<bool> comm_watch_stop{false}, comm_failed{false};
    std::atomic<bool> comm_inflight[kCommSlots] = {}; int64_t comm_enq_ns[kCommSlots] = {0};
    std::string comm_error; int64_t comm_timeout_ms = 600000;
    float *d_params = nullptr, *d_grads = nullptr;                        // views: the caller's ext_params / ext_grads, or ...
    DeviceBuf<float> own_params, own_grads;                               // ... the model's own
    DeviceBuf<float> d_m, d_v, d_wt, d_w1pad, d_tph[3];
    DeviceBuf<float> d_wino_u; float *d_wino_v = nullptr, *d_wino_m = nullptr;   // Winograd scratch: filters (per model), transformed input / output (arena)
    size_t ufl = 0;                                                       // floats of d_wino_u
    int wino_min_cin = 64;                                              // 3x3 layers with Cin >= this use Winograd; 0 = never
    int wino_tile = 6;                                                    // largest 3x3 output tile: F(6x6,3x3) / F(4x4,3x3) per layer by cost, F(2x2,3x3) fallback
    int wino_fc6 = 1;                                                     // fc6 7x7 as a 2x2 grid of 4x4 sub-filters in the Winograd domain
    int fc6_fft = 1;                                                      // ... and in the fp32 training step: forward + data gradient through 14x14 real-DFT tiles (fft_fc6.hip)
    int fc6_fft_wgrad = 1;                                                // ... and its weight gradient too: 1 = from fft6_wgrad_min_tiles tiles up, 2 = at any tile count, 0 = F(4x4,4x4)
    int wino_tile_hires = 0, wino_hires_pixels = 0;                       // != 0: 3x3 layers on maps of at least wino_hires_pixels pixels (per image) use at most this tile
    int wino_force_tile = 0;                                              // != 0: every eligible 3x3 layer uses exactly this tile (op-level parity entry point)
    int precision = FCN8S_PREC_F32;                                       // FCN8S_PREC_BF16_FC: forward fc6 / fc7 on the bf16 MFMA
    // fcn8s_freeze_params: the caller promises constant parameters; Winograd-transformed filters are then kept per layer
    bool frozen = false;
    unsigned long long frozen_fp = 0; DeviceBuf<unsigned long long> d_fp;   // fingerprint of the parameter buffer the cached banks were built from
    PinnedBuf<unsigned long long> h_fp; hipEvent_t fp_event = nullptr;      // pinned landing place of the guard's fingerprint, and the event behind its copy
    std::map<std::string, DeviceBuf<float>> u_cache;                     // layer -> transformed filter bank, valid while frozen
    std::map<std::string, DeviceBuf<float>> u_train;                              // layer -> forward filter bank of the current training step: the adjoint data
                                                                         // gradient reads it as a transposed B operand (no second, transposed bank)
    bool fwd_train = false;                                              // forward() is running a training pass
    PassState pass;                                                       // what that pass and the backward pass behind it left for later launches (pass_state.h)
    int deterministic = 0;                                                // option: reductions split over blocks are joined in a fixed order (slabs + ordered sum) instead of atomics
    int fuse_dgrad_dout = 1;                                              // option: allow that fusion
    int fuse_out_in = 1;                                                  // option: inside a block, conv L's output transform writes conv L+1's V directly (Y is never written): 0 never, 1 unless the row ranges would get too short, 2 always
    int conv1_tiled = 1, conv1_wgrad_mfma = 1;                            // options: conv1_1 forward on the spatial-tile kernel / its weight gradient on the matrix core
    int conv1_in_transform = 1;                                           // option: conv1_1 is evaluated inside conv1_2's input transform (its activation tensor is never written)
    int gemm_out_fused64 = 1;                                             // option: conv1_2 (64 -> 64, F(6x6), its pool the only reader) runs position GEMMs, output transform and pool in one kernel (M is never written); 0 = the two kernels
    int gemm_out64_nt = -1;                                               // op entries (op context "op_gemm_out_fused64" = 2): 1 = wino_gemm_out64_kernel's non-temporal instantiation whatever the size; -1 = the launcher's own rule (every real model)
    int gemm_out64_launches = 0;                                          // launches of wino_gemm_out64_kernel (what fcn8s_op_conv3x3_winograd_pool reports)
    DeviceBuf<unsigned short> d_wbf16;                                    // bf16 copy of one layer's kernel at a time (K-tile-major or transposed)
    std::map<std::string, DeviceBuf<unsigned short>> wbf16_cache;                 // ... per layer, valid while frozen
    // fcn8s_predict_tta on a model that is not frozen keeps the storage of the banks it built (u_cache / wbf16_cache) but not their contents: the keys
    // ("u:<key>" / "w:<key>") whose contents must be rebuilt before use, and whether the first frozen pass must rebuild the padded kernels + fingerprint
    std::set<std::string> bank_stale; bool banks_stale = false;
    int bf16_gemm256 = 1;                                                 // bf16_fc mode: 256 x 256 LDS-DMA kernel -- 0 never, 1 when it fills the chip, 2 whenever shapes allow
    DeviceBuf<unsigned short> d_abf16;                                    // bf16 copy of the layer's input activations
    // bf16 modes, training: zero-bordered padded bf16 copies of the inputs of conv3_1 .. conv5_3, one per layer (the border is written once, at
    // allocation; the interior every step by that layer's Winograd input transform, wino_input_kernel<.., XB>); keyed by layer, dropped with the workspace
    std::map<std::string, DeviceBuf<unsigned short>> xbf16;
    // FCN8S_PREC_BF16_TRAIN: per layer, the zero-bordered bf16 copy of its INPUT with zeroed guard rows in front and behind (bf16_guard_rows), written by
    // the forward pass and read again by the layer's weight gradient
    using G16Map = std::map<std::string, DeviceBuf<unsigned short>>;
    G16Map xg16, dyg16;                                                   // ... per layer: the same kind of copy of its output gradient dY
    std::set<std::string> g16_stale;                                      // ... and which of the two maps' copies ("x:<layer>" / "d:<layer>") carry the zero border of another shape.  It lives and dies with the
                                                                          // copies: drop_shape_copies marks them (fcn8s_predict_tta's re-plans) or clears it with the maps, g16_for zeroes a marked copy on its next use
    int bf16_fuse_pool = 1;                                               // option: bf16_train, the max-pool backward writes the last conv's bf16 dZ copy and bias gradient directly
    int bf16_infer_copies = 1;                                            // option: bf16_train's evaluation / prediction passes take the training pass's data flow (see forward())
    int bf16_rows_bn = 0;                                                 // option (A/B): 128 = the flat-position bf16 convolution takes its 128-column tile where it can (default: 64 columns)
    int bf16_acts = 1;                                                    // option: bf16_train training passes keep a conv -> conv activation only as the consumer's padded bf16 copy (the producer's epilogue writes it; no fp32 tensor, no conversion pass)
    // FCN8S_PREC_FP8_INFER: the calibration (per FP8 layer the max |input| of the fp32 pass; it describes the parameters, not the mode), the device scratch of
    // fcn8s_fp8_calibrate, the e4m3 copies (kept with the workspace) and the weight banks (valid across passes only while frozen: w8_valid)
    bool fp8_calibrated = false; float fp8_amax[FCN8S_FP8_LAYERS] = {}; DeviceBuf<unsigned> d_fp8_amax;
    std::map<std::string, Q8Buf> q8;
    std::map<std::string, W8Bank> w8; std::set<std::string> w8_valid;
    int saved_wino_min_cin = -1, saved_wino_fc6 = -1;                      // the options the mode overrides (the direct path carries it), restored on leaving
    int bf16_copy_by_transform = 1;                                       // option: 0 = every bf16 layer converts its input with a pass of its own (round 3's path)
    int64_t ws_allocs = 0;                                                // statistic "workspace_allocations": device allocations for the workspace, the TTA scratch, the bf16 copies and the cached filter banks
    DeviceBuf<char> crf_buf;                                              // fcn8s_predict_crf: staged images, the mean softmax, the two mean-field buffers, staged output (grown, never shrunk)
    DeviceBuf<char> tta_buf;                                              // fcn8s_predict_tta: staged images, accumulator, staged output (grown, never shrunk)
    DeviceBuf<char> mc_buf;                                               // fcn8s_predict_mc: staged images, the two accumulators, staged outputs (grown, never shrunk)
    bool mc_masks = false;                                                // the last forward pass was fcn8s_predict_mc's: fcn8s_get_dropout_masks reports its last sample's masks
    hipStream_t stream = nullptr;
    // fcn8s_set_stream: every stream the model was given (fcn8s_destroy gives their scratch back) and the event that orders a new stream behind the old one's queue
    std::set<hipStream_t> streams_seen; hipEvent_t move_ev = nullptr;
    int64_t step = 0;
    // workspace for the current (N,H,W)
    int N = 0, H = 0, W = 0;
    int plan_N = 0;
    DeviceBuf<char> arena;
    std::map<std::string, Act> acts;
    std::vector<Layer> layers;                                            // the encoder's weighted layers under the current plan (struct Layer)
    // option "keep_output_gradients" (tests): every weighted layer's fp32 output gradient dY, copied as the backward pass hands it to the layer's weight gradient;
    // read back through fcn8s_get_activation("dy:<layer>")
    struct KeptDy { DeviceBuf<float> p; size_t n = 0; };                  // (n = 0: this pass handed the layer's dY over in another form)
    int keep_dy = 0; std::map<std::string, KeptDy> kept_dy;
    // the last transposed conv (k = 2s = 16) as one GEMM over output blocks (PixMap, elementwise.hip): logits / dlogits live in that blocked layout
    int tconv_gemm = 1; PixMap pm{0, 0, 0, 0, 0, 0}; int tg_kp = 0;
    float *logits_b = nullptr, *dlogits_b = nullptr, *tg_A = nullptr, *tg_dA = nullptr;      // arena
    DeviceBuf<float> tg_b2, tg_b2t, tg_bias, tg_db2;                                          // per model
    bool logits_nhwc_valid = false;
    float *dlogits = nullptr, *da3 = nullptr, *da4 = nullptr, *ds7 = nullptr, *gskip3 = nullptr, *gskip4 = nullptr;
    float *gbuf[2] = {nullptr, nullptr};
    int gcur = 0;
    void* d_images = nullptr; uint8_t* d_labels = nullptr;
    DeviceBuf<float> d_loss; float *d_regsum = nullptr, *d_softmax = nullptr;       // (d_regsum, d_lastbias, d_terms: views into d_loss)
    PinnedBuf<float> h_loss; hipEvent_t loss_ev = nullptr; bool loss_copied = false;   // pinned copy of d_loss, queued right after the loss kernels
    float* d_lastbias = nullptr;       // column sums of dlogits (gradient of the last transposed conv's bias), produced by the loss kernel
    double* d_partials = nullptr; long long* d_pred = nullptr;
    // fcn8s_set_loss: the training loss (0 = the reference's mean, 1 = class-weighted, 2 = OHEM); weights in d_cw (float[64], made once by
    // fcn8s_set_loss); loss_ws = LOSS_SCRATCH_BYTES of state and histograms + (OHEM) the l_p buffer, grown on first use (a "workspace_allocation")
    int loss_mode = 0, last_loss_mode = 0; float ohem_thresh = 0.f; int64_t ohem_min_kept = 0;
    DeviceBuf<float> d_cw; DeviceBuf<char> loss_ws;
    // fcn8s_set_boundary_loss: bnd_R = the radius (0 = off); the 256 weights per distance code in d_btab (made by fcn8s_set_boundary_loss); d_bcodes =
    // the [N, H, W] codes of the training loss's labels, written in front of every such loss (grown on first use, a "workspace_allocation");
    // bnd_last: the pixels of the codes the last training loss wrote, 0 = it ran without the weighting (fcn8s_get_boundary_codes).  With loss_mode == 0 the loss runs the weighted mode
    // on unit class weights: whoever of fcn8s_set_loss / fcn8s_set_boundary_loss leaves that state writes the ones into d_cw
    int bnd_R = 0; long long bnd_last = 0; DeviceBuf<float> d_btab; DeviceBuf<uint8_t> d_bcodes;
    // fcn8s_set_lovasz: L = lov_ce * (the cross-entropy above) + lov_w * L_lov + L2 (lov_on: not the default (1, 0)); the class mask in d_lovmask
    // (uint8[64], made by fcn8s_set_lovasz); lov_ws = the sort's scratch (LovaszLayout), grown on first use (a "workspace_allocation");
    // d_terms = the unscaled terms of the last training loss (ce, lovasz, l2; right behind d_lastbias), have_terms once a training loss ran
    bool lov_on = false, have_terms = false; float lov_ce = 1.f, lov_w = 0.f; int lov_per_image = 0, lov_all = 0;
    DeviceBuf<uint8_t> d_lovmask; int lov_nmask = 0; DeviceBuf<char> lov_ws; float* d_terms = nullptr;
    // fcn8s_set_soft_targets: L += kd_w * L_kd at temperature kd_T over the valid pixels (kd_all: over every pixel); kd_w == 0: off.  kd_probs = the
    // caller's target rows bound by fcn8s_bind_soft_targets (not owned; kd_K floats every kd_stride, for a batch of kd_N x kd_H x kd_W), nullptr once a
    // training loss has consumed them.  kd_ws = the per-block partials, grown on first use (a "workspace_allocation"); the term lands in d_terms[3];
    // have_kd: the last training loss ran with the term
    float kd_w = 0.f, kd_T = 1.f; int kd_all = 0; bool have_kd = false;
    const float* kd_probs = nullptr; int kd_N = 0, kd_H = 0, kd_W = 0, kd_K = 0; long long kd_stride = 0;
    DeviceBuf<char> kd_ws;
    // fcn8s_set_entropy_term: L += ent_w * L_ent over the pixel set ent_set of the images >= ent_first, ent_K logical classes; ent_w == 0: off.
    // ent_ws = the per-block partials, grown on first use (a "workspace_allocation"); the term lands in d_terms[4]; have_ent: the last training
    // loss ran with the term
    float ent_w = 0.f; int ent_set = 0, ent_K = 0, ent_first = 0; bool have_ent = false;
    DeviceBuf<char> ent_ws;
    // fcn8s_set_focal: focal_gamma > 0: the focal launch (focal.hip) stands where the cross-entropy's stands in a training loss; 0: off.  focal_ws = the
    // per-block partials, grown on first use (a "workspace_allocation")
    float focal_gamma = 0.f;
    DeviceBuf<char> focal_ws;
    // fcn8s_accumulate_bucket: the accumulator (total floats, the gradient buffer's buckets; grown at the first fold -- a "workspace_allocation" --
    // and kept until the model goes), per bucket the micro-batches folded and not yet flushed, and whether this backward pass's bucket was taken
    DeviceBuf<float> d_acc; int acc_k[FCN8S_MAX_BUCKETS] = {0}; bool acc_taken[FCN8S_MAX_BUCKETS] = {false};
    // fcn8s_set_grad_clip: max_norm (0 = off); upd_ws = UpdateStats + the norm's kGradNormBlocks partial sums, made by fcn8s_set_grad_clip;
    // last_update_clipped: the last fcn8s_apply_update ran the norm pass (fcn8s_get_update_stats)
    float max_norm = 0.f; DeviceBuf<char> upd_ws; bool last_update_clipped = false;
    // fcn8s_set_ema: the moving average of the parameters -- the shadow (total floats; grown when the average is first switched on -- a
    // "workspace_allocation" -- and kept until the model goes), its decay (0 = off) and warm-up rule, and whether theta and the shadow have changed places
    DeviceBuf<float> d_ema; double ema_decay = 0.0; int ema_warmup = 1; bool ema_swapped = false;
    DeviceBuf<unsigned long long> d_conf;
    double loss_sum = 0; int64_t loss_cnt = 0;
    float keep_prob = 1.f, l2_rate = 0.f;
    uint32_t drop_stream = 0;
    bool have_forward = false, have_loss = false, train_mode = false;
    int next_bucket = 0;
    const uint8_t* cur_labels = nullptr;
    bool profile = false, profile_detail = false;
    // pinned host staging + device slots filled on a copy stream (fcn8s_stage_inputs): the next batch's H2D overlaps this step's kernels
    struct StageSlot { PinnedBuf<uint8_t> h_img, h_lab; DeviceBuf<uint8_t> d_img, d_lab;
                       hipEvent_t ready = nullptr, consumed = nullptr; bool used = false; };
    StageSlot slots[FCN8S_NUM_STAGE_SLOTS];
    hipStream_t copy_stream = nullptr;
    std::vector<ProfGroup> groups;
    std::string err;
    // Memory frees itself (the Buf members above).  Events and the copy stream are destroyed here; the caller has drained the device
    // (fcn8s_destroy) or the stream (the bare models of the fcn8s_op_* entry points) first.
    fcn8s_model() = default;
    fcn8s_model(const fcn8s_model&) = delete;
    ~fcn8s_model()
    {
        for (auto& g : groups) for (auto& ev : g.ev) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
        for (auto& e : bucket_ev) if (e) hipEventDestroy(e);
        if (loss_ev) hipEventDestroy(loss_ev);
        if (move_ev) hipEventDestroy(move_ev);
        if (fp_event) hipEventDestroy(fp_event);
        for (auto& sl : slots) { if (sl.ready) hipEventDestroy(sl.ready); if (sl.consumed) hipEventDestroy(sl.consumed); }
        if (copy_stream) hipStreamDestroy(copy_stream);
    }
};

namespace {

int fail(fcn8s_model* m, int code, const std::string& msg)
{
    if (m) m->err = msg;
    g_last_error = msg;
    return code;
}
// what a launcher recorded with defer_error during the call that is about to return (0: nothing)
int deferred_rc(fcn8s_model* m)
{
    std::string t; const int c = take_deferred_error(&t);
    return c ? fail(m, c, t) : FCN8S_OK;
}
#define HIPCHK(m, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return fail(m, e_ == hipErrorOutOfMemory ? FCN8S_ERR_OOM : FCN8S_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

const int kNumBuckets = 4;      // (what fcn8s_num_buckets reports; callers size nothing by a compile-time constant)
const size_t kUpdPartialsOff = 32;      // fcn8s_model::upd_ws: UpdateStats, then (from this byte on) the norm pass's partial sums

void build_param_table(int C, const int widths[7], int fc6k, std::vector<ParamInfo>& out, size_t& total,
                       size_t boff[FCN8S_MAX_BUCKETS], size_t bn[FCN8S_MAX_BUCKETS])
{
    out.clear();
    size_t off = 0;
    auto add = [&](const std::string& name, std::initializer_list<int64_t> shp) {
        ParamInfo p; p.name = name; p.ndim = (int)shp.size(); p.numel = 1;
        int i = 0; for (auto s : shp) { p.shape[i++] = s; p.numel *= (size_t)s; }
        for (; i < 4; ++i) p.shape[i] = 1;
        p.offset = off; off = align_up(off + p.numel, 64);   // 256-byte aligned tensors
        out.push_back(p);
    };
    int cin = 3;
    size_t conv4_start = 0, fc6_start = 0, fc7_start = 0;
    for (int b = 0; b < 5; ++b)
        for (int i = 1; i <= kConvsPerBlock[b]; ++i) {
            char nm[32]; snprintf(nm, sizeof nm, "conv%d_%d", b + 1, i);
            if (b == 3 && i == 1) conv4_start = off;
            add(std::string(nm) + "/filter", {3, 3, cin, widths[b]});
            add(std::string(nm) + "/biases", {widths[b]});
            cin = widths[b];
        }
    fc6_start = off;
    add("fc6/weights", {fc6k, fc6k, widths[4], widths[5]});
    add("fc6/biases", {widths[5]});
    fc7_start = off;
    add("fc7/weights", {1, 1, widths[5], widths[6]});
    add("fc7/biases", {widths[6]});
    add("pool3_1x1/kernel", {1, 1, widths[2], C});
    add("pool3_1x1/bias", {C});
    add("pool4_1x1/kernel", {1, 1, widths[3], C});
    add("pool4_1x1/bias", {C});
    add("fc7_1x1/kernel", {1, 1, widths[6], C});
    add("fc7_1x1/bias", {C});
    add("fc7_conv2d_trans/kernel", {4, 4, C, C});
    add("fc7_conv2d_trans/bias", {C});
    add("fc7_pool4_conv2d_trans/kernel", {4, 4, C, C});
    add("fc7_pool4_conv2d_trans/bias", {C});
    add("fc7_pool4_pool3_conv2d_trans/kernel", {16, 16, C, C});
    add("fc7_pool4_pool3_conv2d_trans/bias", {C});
    total = off;
    // gradient buckets = contiguous slices in backward-production order: {fc7, decoder} (68 MB, final first) | {fc6} (411 MB) |
    // {conv4, conv5} (52 MB) | {conv1..conv3} (7 MB).  fc6 has a bucket of its own so that the exchange of the other 68 MB of the head does
    // not wait for the 3 ms of fc6's weight-gradient GEMMs, and fc6's own starts the moment they end (round 3 had one 479 MB bucket).
    for (int i = 0; i < FCN8S_MAX_BUCKETS; ++i) { boff[i] = 0; bn[i] = 0; }
    boff[0] = fc7_start;   bn[0] = total - fc7_start;
    boff[1] = fc6_start;   bn[1] = fc7_start - fc6_start;
    boff[2] = conv4_start; bn[2] = fc6_start - conv4_start;
    boff[3] = 0;           bn[3] = conv4_start;
}

void resolve_cfg(const fcn8s_config* cfg, int& C, int widths[7], int& fc6k)
{
    static const int def[7] = {64, 128, 256, 512, 512, 4096, 4096};
    C = cfg->num_classes;
    fc6k = cfg->fc6_ksize > 0 ? cfg->fc6_ksize : 7;
    for (int i = 0; i < 7; ++i) widths[i] = cfg->widths[i] > 0 ? cfg->widths[i] : def[i];
}

const ParamInfo& P(const fcn8s_model* m, const std::string& n) { return m->params[m->index.at(n)]; }
float* Wp(fcn8s_model* m, const std::string& n) { return m->d_params + P(m, n).offset; }
float* Gp(fcn8s_model* m, const std::string& n) { return m->d_grads + P(m, n).offset; }
float* WTp(fcn8s_model* m, const std::string& n) { return m->d_wt + P(m, n).offset; }

// ---- profiling wrappers -------------------------------------------------------
int group_id(fcn8s_model* m, const char* name)
{
    for (size_t i = 0; i < m->groups.size(); ++i) if (m->groups[i].name == name) return (int)i;
    ProfGroup g; g.name = name; m->groups.push_back(g);
    return (int)m->groups.size() - 1;
}
struct ProfScope {
    fcn8s_model* m; int gid = -1; hipEvent_t a = nullptr, b = nullptr; double fl = 0, by = 0;
    ProfScope(fcn8s_model* m_, const char* group, double flops, double bytes, const char* layer = nullptr) : m(m_), fl(flops), by(bytes)
    {
        if (!m || !m->profile) return;          // (no model: an op-level entry point, nothing to profile)
        fcn8s::g_last_kernel = nullptr;
        gid = (m->profile_detail && layer) ? group_id(m, (std::string(group) + ":" + layer).c_str()) : group_id(m, group);
        hipEventCreate(&a); hipEventCreate(&b);
        hipEventRecord(a, m->stream);
        m->groups[gid].flops += flops; m->groups[gid].bytes += bytes; m->groups[gid].launches += 1;
    }
    ~ProfScope()
    {
        if (gid < 0) return;
        hipEventRecord(b, m->stream);
        m->groups[gid].ev.emplace_back(a, b);
        if (fcn8s::g_last_kernel) {          // second view of the same launch, keyed by the kernel symbol that ran
            const int k = group_id(m, (std::string("kernel:") + fcn8s::g_last_kernel).c_str());
            m->groups[k].flops += fl; m->groups[k].bytes += by; m->groups[k].launches += 1;
            m->groups[k].ev_shared.emplace_back(a, b);
        }
    }
};

// A count-only group of the detailed profile (fcn8s_profile_enable(m, 2)), "derived:<build step>": a FORWARD pass (re)built one more tensor from
// the parameters alone -- a Winograd filter bank, a bf16 relayout of a kernel, the padded / phase-packed kernels.  No events, no time (ms, flops
// and bytes stay 0: consumers that divide by ms skip such groups): what a frozen model's later passes must report as zero (fp8_infer's banks
// have a timed group of their own, fp8_quantize_w).  The name is written at the build site, so a new build site needs its own line.
static void prof_derived(fcn8s_model* m, const char* what)
{
    if (m && m->profile && m->profile_detail) m->groups[group_id(m, (std::string("derived:") + what).c_str())].launches += 1;
}

// ---- layer launchers ------------------------------------------------------------
struct ConvEpi { float alpha = 1.f; };                   // both directions: the product is scaled by alpha before the epilogue
struct FwdEpi : ConvEpi {
    const float* bias = nullptr; int relu = 0;
    int dropout = 0; float keep = 1.f; uint32_t stream_id = 0;      // dropout behind the ReLU (fc6 / fc7): keep probability, counter stream of its random numbers
    float* pool_out = nullptr; unsigned char* pool_idx = nullptr;   // 2x2/2 max-pool of the output, written by the Winograd output transform if that path runs, with the per-window argmax bytes the backward pass routes by
    int skip_y = 0;                                      // Winograd path with pool_out: do not write the full-resolution output (only its pool is consumed)
    unsigned* relu_bits_out = nullptr;                   // Winograd path: also record (y > 0), one bit per element
    unsigned* in_relu_bits_out = nullptr; const char* in_layer = nullptr;   // Winograd path: record (x > 0) of the input too (wino_input_kernel), under this producer's name in pass.rbits_ok
    float* next_v = nullptr; const char* next_layer = nullptr;     // Winograd F(6x6) path: write the NEXT conv's V here instead of this conv's output, and promise it to that conv (pass.fwd_v)
    bool gemm_out_fused64 = false;                       // the layer's rule gemm_out_fused64 holds and option "gemm_out_fused64" is on: position GEMMs + output transform + pool in one kernel where this launch allows it (conv_winograd)
};
struct DgradEpi : ConvEpi {
    const float* addend = nullptr;                       // added to dX (the skip paths' gradients)
    const float* mask = nullptr; float mask_scale = 1.f; // dX *= (mask > 0) * mask_scale: the ReLU / dropout of the layer's input
    const unsigned* relu_bits_in = nullptr;              // Winograd path: the bit record of (mask > 0), read instead of the tensor
    const float* w_fwd = nullptr;                        // the layer's forward kernel [K,K,Cout here,Cin here] (adjoint Winograd paths, bf16_train)
    int lazy_wt = 0;                                     // `w` is still to be filled from w_fwd (flip + transpose) if no path that reads w_fwd is taken
    float* dm_out = nullptr; const char* dm_out_layer = nullptr;   // adjoint path: write dM of the producing layer here instead of its dZ into y, and promise it to that layer's weight gradient (pass.dm_prefilled)
    const char* yb_layer = nullptr; int yb_K = 3;        // bf16_train: the layer whose output gradient this launch produces, and its kernel size
    bool yb_only = false;                                // ... both of that layer's gradients take its bf16 copy (dy_bf16_only): write the copy, the fp32 tensor stays unwritten
};

// 3x3 SAME conv through Winograd F(tile x tile, 3x3): filter transform, input transform, (tile+2)^2 batched GEMMs
// on the matrix cores (2.25x / 4x fewer MFMA flops than the direct form), output transform + fused epilogue.
// u: [P][Cin][Cout], v: [P][T][Cin], mm: [P][T][Cout] scratch, P = (tile+2)^2, T = N*(H/tile)*(W/tile).
// Which layer takes it, with which tile and which fusions: conv_route.h.
// Arithmetic of the op-level entry points, which have no model: the context of the CALLING THREAD (fcn8s_set_option(NULL, "op_split_pieces", n)
// from that thread), copied into the bare model each such call builds -- never read by a real model, never shared between threads.
thread_local int t_op_split = 0;
thread_local int t_op_rows_bn = 0;       // op context: the form of the flat-position 3 x 3 kernel fcn8s_op_conv2d_bf16_train asks for (option "op_bf16_rows_bn")
thread_local int t_op_fused64 = 0;       // op context: fcn8s_op_conv3x3_winograd_fwd_bwd / _pool ask for wino_gemm_out64_kernel (option "op_gemm_out_fused64": 1, 2 = its non-temporal instantiation)
thread_local int t_op_planes = 1;        // op context: fcn8s_op_conv2d_bf16_train keeps its padded copies as channel-chunk planes (option "op_bf16_planes")
int split_of(const fcn8s_model* m)
{
    if (!m) return t_op_split;
    if (m->precision == FCN8S_PREC_F32X3 || m->precision == FCN8S_PREC_BF16_FWD) return 3;
    if (m->precision == FCN8S_PREC_F32X2 || m->precision == FCN8S_PREC_BF16_FWD_X2) return 2;
    return 0;
}
static inline bool bf16_fwd_mode(const fcn8s_model* m) { return m->precision == FCN8S_PREC_BF16_FWD || m->precision == FCN8S_PREC_BF16_FWD_X2; }
static inline bool bf16_train_mode(const fcn8s_model* m) { return m && m->precision == FCN8S_PREC_BF16_TRAIN; }
// guard rows of a padded bf16 copy that the weight-gradient kernel reads (gemm_bf16.hip): the largest tap shift + one K-tile of rounding
// (... and, for the nine-tap kernel, the eight-row instruction that completes a 34-row group: 128 rows cover all of it)
//  ... and conv_bf16_r64_kernel's last row tile, which runs up to 255 positions past the last one and reads 272 rows from one filter row above it: 640)
static inline long long bf16_guard_rows(int K, int Wp) { return (long long)((K - 1) / 2) * Wp + (K - 1) / 2 + 640; }
// bf16_train's per-layer padded copies are stored as channel-chunk PLANES [C / 32][guard + rows + guard][32] (Bf16Conv256Args): elements between two planes
#ifndef A_PLANES
#define A_PLANES 1                   // (0: the copies as [rows][C] -- the A/B switch of tools/ab_variants.sh; every kernel takes both)
#endif
static inline long long g16_ps(int N, int H, int W, int K) { const int pad = (K - 1) / 2, Wp_ = W + 2 * pad; return A_PLANES ? ((long long)N * (H + 2 * pad) * Wp_ + 2 * bf16_guard_rows(K, Wp_)) * 32 : 0; }
static inline long long g16_off(long long G, int C) { return A_PLANES ? G * 32 : G * C; }      // elements from the start of a copy's buffer to its padded pixel 0
unsigned short* g16_for(fcn8s_model* m, fcn8s_model::G16Map& bufs, const char* layer, int N, int H, int W, int C, int K, hipStream_t s);
unsigned short* dyb_for(fcn8s_model* m, const char* layer, const float* dy, int N, int H, int W, int C, int K, hipStream_t s, float* db = nullptr, bool* db_done = nullptr);

// The one place an fcn8s_model becomes the options of conv_route.h (a null model -- the op entry points without a context -- has no Winograd route).
// The bare models of the fcn8s_op_* entry points come through here like any other.
RouteOpts route_opts(const fcn8s_model* m)
{
    RouteOpts o;
    if (!m) { o.wino_min_cin = 0; o.wino_fc6 = 0; return o; }
    o.wino_min_cin = m->wino_min_cin; o.wino_tile = m->wino_tile; o.wino_tile_hires = m->wino_tile_hires; o.wino_hires_pixels = m->wino_hires_pixels;
    o.wino_force_tile = m->wino_force_tile; o.wino_fc6 = m->wino_fc6; o.plan_N = m->plan_N; o.scratch = m->d_wino_v != nullptr;
    return o;
}
int wino_tile_for(const fcn8s_model* m, int H, int W, int K = 3) { return m ? wino_tile_for(route_opts(m), H, W, K) : 0; }
// ... and the per-launch options of its bf16_train rules, for a training (train) or an evaluation / prediction pass of a model in that mode
Bf16Opts bf16_opts(const fcn8s_model* m, bool train)
{
    Bf16Opts o; o.acts = m->bf16_acts != 0; o.fuse_pool = m->bf16_fuse_pool != 0; o.conv1_tiled = m->conv1_tiled != 0; o.copies = train || m->bf16_infer_copies != 0;
    return o;
}
long long wino_tiles(int tile, int N, int H, int W) { return (long long)N * ((H + tile - 1) / tile) * ((W + tile - 1) / tile); }
struct WinoEpi { const float* bias = nullptr; const float* addend = nullptr; const float* mask = nullptr; float mask_scale = 1.f;
                 int relu = 0; int dropout = 0; float keep = 1.f; unsigned long long seed = 0; unsigned int stream_id = 0; float* pool = nullptr; unsigned char* pidx = nullptr;
                 unsigned* rbits_out = nullptr; const unsigned* rbits_in = nullptr; int skip_y = 0;
                 unsigned* in_rbits_out = nullptr;       // ReLU bit record of the INPUT, written by the input transform
                 float* next_v = nullptr; bool* fused_out = nullptr;        // output transform fused with the next conv's input transform (winograd.hip: wino_out_in_kernel)
                 bool gemm_out_fused64 = false; };                          // rule gemm_out_fused64 and its option: see conv_winograd
// fc6 through 14x14 real-DFT tiles (fft_fc6.hip) in the fp32 training step of an unfrozen model.  Frozen inference keeps its cached
// F(4x4,4x4) bank (at batch 1 the 2.45 GB DFT bank would cost more than it saves), the other precisions keep their own fc6 paths, and the
// weight gradient stays in F(4x4,4x4) (V of pool5 is written here for it).  ci / co: channels of the FORWARD conv.
// Only on maps where the DFT tiles multiply less than the alternative (per image: 292 planes per 8x8 tile against F(4x4,4x4)'s 196 per 4x4 tile,
// or 49 per output for the direct form): at the training shape (32x16) 2336 against 6272; a 2x2 map (64x64 images) keeps F(4x4,4x4), 196 against 292.
static bool fft6_cheaper(const fcn8s_model* m, int H, int W)
{
    const long long fft = 292LL * ((H + 7) / 8) * ((W + 7) / 8);
    const long long other = wino_tile_for(m, H, W, 7) == 4 ? 196LL * (H / 4) * (W / 4) : 49LL * H * W;
    return fft < other;
}
static bool fft6_shape_ok(const fcn8s_model* m, int ci, int co) { return m->wino_fc6 && m->fc6_fft && m->fc6k == 7 && ci % 16 == 0 && co % 128 == 0; }
static bool fft6_on(const fcn8s_model* m, int N, int H, int W, int ci, int co)
{
    if (!m || !fft6_shape_ok(m, ci, co) || !fft6_cheaper(m, H, W) || m->precision != FCN8S_PREC_F32 || m->frozen || !m->d_wino_v || !m->d_wino_m) return false;
    const long long T = fft_fc6_tiles(N, H, W);
    auto v = m->acts.find("wino_v"), mm = m->acts.find("wino_m");
    // (V holds Xf / dXf, ci channels; M holds Yf / dYf, co channels, then the patch gradients, ci channels -- whichever of ci, co is the larger)
    return v != m->acts.end() && mm != m->acts.end() && v->second.n >= (size_t)fft_fc6_planes() * (size_t)wino_slab(T, ci) &&
           mm->second.n >= std::max((size_t)fft_fc6_planes() * (size_t)wino_slab(T, co), (size_t)T * 196 * ci);
}
// The weight gradient in the DFT domain (dUf[p] = Xf[p]^T dYf[p], dW = filter^T(dUf)) multiplies 4.56 times per tile position and channel pair
// against F(4x4,4x4)'s 12.25, but writes and reads a 292-plane bank of Cin x Cout (2.45 GB at 512 -> 4096) where F(4x4,4x4) has 196 planes:
// a fixed cost per step that only enough tiles pay for.  Both costs scale with Cin x Cout, so the rule is a tile count.  Measured at 1024x512,
// 512 -> 4096 (tools/layer_bench.py, whole step, DFT against F(4x4,4x4); profiles/r07_fc6_wgrad_tile_sweep.txt): T = 8 (one image) +0.24 ms,
// T = 16 +0.04 ms, T = 32 -0.08 ms, T = 64 -0.65 ms, T = 128 (the bench shape) -0.8 ms.
constexpr long long kFft6WgradMinTiles = 32;
static bool fft6_wgrad_wanted(const fcn8s_model* m, long long T) { return m->fc6_fft_wgrad == 2 || (m->fc6_fft_wgrad == 1 && T >= kFft6WgradMinTiles); }
// fc6's share of the scratch for N maps of h5 x w5 (ci -> co channels), in floats; plan_workspace and fcn8s_op_conv7x7_fc6_fwd_bwd size by it.
//   v_wino        : V / M of F(4x4,4x4) (the data gradient swaps the two roles; M has nsub = 1)
//   v_fft, m_fft  : the DFT tiles: Xf / dXf in V, Yf / dYf and the patch gradients in M
//   wv            : the layer's own slot: V of F(4x4,4x4) or, when the weight gradient runs in the DFT domain, Xf -- sized for either
struct Fc6Scratch { size_t v_wino = 0, v_fft = 0, m_fft = 0, wv = 0; };
static Fc6Scratch fc6_scratch_floats(const fcn8s_model* m, int N, int h5, int w5, int ci, int co)
{
    Fc6Scratch r;
    const int hi = std::max(ci, co);
    if (m->fc6k == 7 && wino_shape_tile(route_opts(m), ConvShape{N, h5, w5, ci, co, 7}) == 4) {
        const size_t P = (size_t)wino_alpha(4, 7) * wino_alpha(4, 7);
        const int ns2 = wino_nsub(7) * wino_nsub(7);
        const long long T = wino_tiles(4, N, h5, w5);
        r.v_wino = std::max(P * (size_t)wino_slab(T, ns2 * hi), P * (size_t)wino_slab(T, hi));
        r.wv = P * (size_t)wino_slab(T, ns2 * ci);
    }
    if (fft6_shape_ok(m, ci, co) && fft6_cheaper(m, h5, w5)) {
        const size_t P = (size_t)fft_fc6_planes();
        const long long T = fft_fc6_tiles(N, h5, w5);
        r.v_fft = P * (size_t)wino_slab(T, ci);
        r.m_fft = std::max(P * (size_t)wino_slab(T, co), (size_t)T * 196 * ci);
        if (fft6_wgrad_wanted(m, T)) r.wv = std::max(r.wv, P * (size_t)wino_slab(T, ci));
    }
    return r;
}
// ... and of the filter-bank scratch d_wino_u: 49 positions x 4 sub-filters, or the 292 planes of the DFT-domain weight gradient (dUf; +0.8 GB at 512 -> 4096)
static size_t fc6_bank_floats(int ci, int co)
{
    size_t n = 49 * 4 * (size_t)ci * co;
    if (ci % 16 == 0 && co % 128 == 0) n = std::max(n, (size_t)fft_fc6_planes() * ci * co);
    return n;
}
// One batched GEMM per transform position (a DFT plane, a Winograd position): [T x K] x [K x Nc] per position, the slabs wino_slab() apart.
// split, fixed_tile and a transposed B operand (bt, ldw) are the caller's.  fc6's DFT planes take fixed_tile = 1: 128-row tiles and no
// split-K whatever the batch (a DP shard computes the big batch's bits)
static IgemmArgs position_gemm(const float* x, const float* w, float* y, long long T, int K, int Nc)
{
    IgemmArgs a{};
    a.x = x; a.w = w; a.y = y;
    a.N = 1; a.Ma = (int)T; a.Mb = 1; a.M = T;
    a.Hi = (int)T; a.Wi = 1; a.Cin = K; a.ldx = K;
    a.KW = 1; a.in_scale = 1; a.tap_step = 1; a.tap_off = 0; a.Ktot = K;
    a.Ho = (int)T; a.Wo = 1; a.Cout = Nc; a.ldy = Nc;
    a.out_scale = 1; a.phases_x = 1; a.w_phase_stride = (long long)K * Nc;
    a.alpha = 1.f; a.mask_scale = 1.f;
    a.batched = 1; a.x_batch_stride = wino_slab(T, K); a.y_batch_stride = wino_slab(T, Nc);
    return a;
}
// ... and its weight-gradient twin: C[p] = A[p]^T B[p] over the T rows of a position, [Kg x Cout] per position, every element written once (plain stores,
// no bias sums).  split is the caller's.
static WgradArgs position_wgrad(const float* A, const float* B, float* C, long long T, int Kg, int Cout, int positions)
{
    WgradArgs g{};
    g.A = A; g.B = B; g.C = C;
    g.N = 1; g.Pa = 1; g.Pb = (int)T; g.P = T;
    g.Ha = 1; g.Wa = (int)T; g.Adim = Kg; g.lda = Kg; g.Areal = Kg;
    g.Bdim = Cout; g.ldb = Cout; g.KW = 1; g.a_scale = 1; g.tap_off = 0; g.ntaps = positions; g.ldc = Cout; g.alpha = 1.f; g.colsum = nullptr;
    g.batched = 1; g.a_batch_stride = wino_slab(T, Kg); g.b_batch_stride = wino_slab(T, Cout); g.c_uninitialized = 1;
    return g;
}
// forward: Uf (kept for the data gradient), Xf, the 292 plane GEMMs, the output transform with fc6's epilogue.  false: not taken (no bank memory)
static bool conv_fft6_fwd(fcn8s_model* m, const char* layer, const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout,
                          const float* bias, int relu, int dropout, float keep, unsigned int stream_id, hipStream_t s)
{
    const int P = fft_fc6_planes();
    const long long T = fft_fc6_tiles(N, H, W);
    DeviceBuf<float>& uf = m->u_train[std::string(layer) + "#fft"];
    if (!uf.grow((size_t)P * Cin * Cout * sizeof(float), s)) return false;
    auto wv = m->acts.find(std::string("wv:") + layer);      // the weight gradient's input operand: Xf (DFT domain) or V of F(4x4,4x4)
    // the DFT-domain weight gradient reads this pass's Xf: kept in the layer's own slot, which nothing else writes before the backward pass
    const bool dft_wgrad = wv != m->acts.end() && fft6_wgrad_wanted(m, T) && wv->second.n >= (size_t)P * (size_t)wino_slab(T, Cin) &&
                           m->ufl >= (size_t)P * Cin * Cout;
    const bool want_v = !dft_wgrad && wv != m->acts.end() && wino_tile_for(m, H, W, 7) == 4;
    float* xf = dft_wgrad ? wv->second.p : m->d_wino_v;
    { ProfScope ps(m, "fc6_fft_transform", 0, 4.0 * ((49.0 + P) * Cin * Cout + (double)N * H * W * Cin + (double)P * T * Cin));
      launch_fft_fc6_filter(w, uf, Cin, Cout, s); launch_fft_fc6_input(x, xf, N, H, W, Cin, s); }
    if (want_v) { ProfScope ps(m, "wino_transform", 0, 4.0 * ((double)N * H * W * Cin * 4 + 49.0 * wino_tiles(4, N, H, W) * 4 * Cin));
                  launch_wino_input(4, x, wv->second.p, N, H, W, Cin, 7, s); }
    IgemmArgs a = position_gemm(xf, uf, m->d_wino_m, T, Cin, Cout); a.fixed_tile = 1;
    { ProfScope ps(m, "fc6_fft_gemm_fwd", 2.0 * P * T * Cin * Cout, 4.0 * P * (T * (double)(Cin + Cout) + (double)Cin * Cout), layer); launch_igemm(a, P, s); }
    { ProfScope ps(m, "fc6_fft_transform", 0, 4.0 * ((double)P * T * Cout + (double)N * H * W * Cout));
      launch_fft_fc6_output(m->d_wino_m, bias, y, N, H, W, Cout, relu, dropout, keep, m->seed, stream_id, s); }
    m->pass.fft6_ready.give(layer);
    if (dft_wgrad) m->pass.fft6_xf.give(layer);
    return true;
}
// weight gradient (Cin / Cout: channels of the forward conv): dYf = output^T(dz) into d_wino_m, where the data gradient then finds it;
// dUf[p] = Xf[p]^T dYf[p] over the T tiles (292 planes, one K-slab: every element of dUf has one writer, plain stores); dW = filter^T(dUf);
// the bias gradient is the column sum of dz
static void conv_fft6_wgrad(fcn8s_model* m, const char* layer, const float* xf, const float* dz, float* dw, float* db, int N, int H, int W, int Cin, int Cout, hipStream_t s)
{
    const int P = fft_fc6_planes();
    const long long T = fft_fc6_tiles(N, H, W);
    { ProfScope ps(m, "fc6_fft_transform", 0, 4.0 * ((double)N * H * W * Cout + (double)P * T * Cout)); launch_fft_fc6_dout(dz, m->d_wino_m, N, H, W, Cout, s); }
    m->pass.fft6_dyf.give(layer);
    WgradArgs g = position_wgrad(xf, m->d_wino_m, m->d_wino_u, T, Cin, Cout, P); g.split = 0;
    { ProfScope ps(m, "fc6_fft_gemm_wgrad", 2.0 * P * T * Cin * Cout, 4.0 * P * (T * (double)(Cin + Cout) + (double)Cin * Cout), layer); launch_wgrad(g, s); }
    { ProfScope ps(m, "fc6_fft_transform", 0, 4.0 * (P + 49.0) * Cin * Cout); launch_fft_fc6_dfilter(m->d_wino_u, dw, Cin, Cout, s); }
    if (db) { ProfScope ps(m, "colsum", 0, 4.0 * N * H * W * Cout); launch_colsum(dz, db, (long long)N * H * W, Cout, s); }
}
// data gradient (Cdy / Cdx: channels of dz / of dx): dYf = output^T(dz), dXf[p] = dYf[p] Uf[p]^T with this step's bank read
// transposed, dx = input^T(dXf) (patch gradients, then the overlap-add gather)
static void conv_fft6_dgrad(fcn8s_model* m, const char* layer, const float* dz, const float* uf, float* dx, int N, int H, int W, int Cdy, int Cdx, hipStream_t s)
{
    const int P = fft_fc6_planes();
    const long long T = fft_fc6_tiles(N, H, W);
    if (!m->pass.fft6_dyf.take(layer)) {     // (else the weight gradient just wrote dYf of this dz into d_wino_m)
        m->pass.fft6_dyf.drop();
        ProfScope ps(m, "fc6_fft_transform", 0, 4.0 * ((double)N * H * W * Cdy + (double)P * T * Cdy)); launch_fft_fc6_dout(dz, m->d_wino_m, N, H, W, Cdy, s);
    }
    IgemmArgs a = position_gemm(m->d_wino_m, uf, m->d_wino_v, T, Cdy, Cdx);
    a.fixed_tile = 1; a.bt = 1; a.ldw = Cdy;
    { ProfScope ps(m, "fc6_fft_gemm_dgrad", 2.0 * P * T * Cdy * Cdx, 4.0 * P * (T * (double)(Cdy + Cdx) + (double)Cdy * Cdx), layer); launch_igemm(a, P, s); }
    { ProfScope ps(m, "fc6_fft_transform", 0, 4.0 * ((double)P * T * Cdx + 2.0 * 196.0 * T * Cdx + (double)N * H * W * Cdx));
      launch_fft_fc6_din(m->d_wino_v, m->d_wino_m, dx, N, H, W, Cdx, s); }
}

// KS = 3, or 7 (3x3 grid of 3x3 sub-filters, GEMM depth 9*Cin -- see winograd.hip).  fwd: a forward convolution (its filter bank is kept for a
// frozen model / for this step's adjoint data gradient), else the same algorithm as a data gradient on flipped + transposed weights
void conv_winograd(fcn8s_model* m, int tile, int KS, bool fwd, const float* x, const float* wk, float* y, float* u, float* v, float* mm,
                   int N, int H, int W, int Cin, int Cout, const WinoEpi& e, hipStream_t s, const char* layer, bool v_ready = false)
{
    const int P = wino_alpha(tile, KS) * wino_alpha(tile, KS), nsub2 = wino_nsub(KS) * wino_nsub(KS);
    const long long T = wino_tiles(tile, N, H, W);
    const int Kg = nsub2 * Cin;
    IgemmArgs a = position_gemm(v, u, mm, T, Kg, Cout); a.split = split_of(m);
    const double tb = 4.0 * ((double)N * H * W * Cin * nsub2 + (double)P * T * Kg), ob = 4.0 * ((double)N * H * W * Cout * ((e.pool ? (e.skip_y ? 0.25 : 1.25) : 1.0) + (e.rbits_in ? 1.0 / 32 : (e.mask ? 1.0 : 0.0)) + (e.addend ? 1.0 : 0.0) + (e.rbits_out ? 1.0 / 32 : 0.0)) + (double)P * T * Cout);   // y (+ pool) written, ReLU mask / skip addend read
    // frozen parameters (evaluate / predict loops): the transformed filter bank of each forward layer is computed once and kept
    bool u_cached = false;
    // rule gemm_out_fused64 (the caller's e.gemm_out_fused64: the layer's fact and the option): the layer's bank is kept twice, the standard one -- this
    // step's adjoint data gradient reads it -- and, behind it in the same buffer, the copy in wino_gemm_out64_kernel's operand order.  Both are
    // written whenever the bank is, whatever this launch then runs: a cached bank outlives the launch (a frozen model may change its precision).
    const size_t bank = (size_t)P * Kg * Cout;
    const bool bank2 = m && layer && fwd && e.gemm_out_fused64 && tile == 6 && KS == 3 && Cin == 64 && Cout == 64;
    const size_t bank_bytes = (bank + (bank2 ? wino_gemm_out64_bank_floats() : 0)) * sizeof(float);
    size_t u_floats = m && u == m->d_wino_u ? m->ufl : bank;      // floats behind u
    const char* tag = KS == 7 ? (fwd ? "wino_gemm_fc6_fwd" : "wino_gemm_fc6_dgrad") : (fwd ? "wino_gemm_fwd" : "wino_gemm_dgrad");
    if (m && m->frozen && layer && fwd) {
        DeviceBuf<float>& cu = m->u_cache[std::string(layer) + "#" + std::to_string(tile)];       // (the tile, hence the bank's shape, depends on the image size)
        const std::string key = "u:" + std::string(layer) + "#" + std::to_string(tile);
        if (cu && !m->bank_stale.count(key)) { u = cu; u_cached = true; u_floats = cu.elems(); }
        else if (cu) { u = cu; u_floats = cu.elems(); m->bank_stale.erase(key); }           // kept storage: refilled below
        else if (cu.grow(bank_bytes, s, &m->ws_allocs)) { u = cu; u_floats = cu.elems(); }  // filled below, reused from the next call on (out of memory: the shared scratch)
        a.w = u;
    }
    if (m && !u_cached && m->fwd_train && layer && fwd && ((KS == 3 && tile == 6) || (KS == 7 && tile == 4))) {
        DeviceBuf<float>& tu = m->u_train[std::string(layer) + "#" + std::to_string(tile)];
        if (tu.grow(bank_bytes, s)) { u = tu; a.w = u; u_floats = tu.elems(); }
    }
    float* const u64 = bank2 && u_floats >= bank + wino_gemm_out64_bank_floats() ? u + bank : nullptr;
    // What only this launch knows, ANDed with the rule: the fp32 precision (f32x3 / f32x2 and the bf16 modes that reach this layer through Winograd --
    // bf16_fc, bf16_fwd -- keep the arithmetic they were measured and bounded with; bf16_train and fp8_infer never come here), nobody asks for the
    // full-resolution activation, and the plain epilogue bias + ReLU + pool.  Declined: the two kernels, exactly as ever.
    const bool gemm_out64 = u64 && m->precision == FCN8S_PREC_F32 && split_of(m) == 0 && e.pool && e.skip_y && e.bias && e.relu && !e.addend && !e.mask && !e.dropout && !e.rbits_in && !e.rbits_out && !e.next_v;
    // v_ready: V is already written (forward: by the previous conv's fused output transform; data gradient: with the weight gradient's dM)
    auto pre = [&]() { if (!u_cached) { prof_derived(m, "wino_filter_kernel"); launch_wino_filter(tile, wk, u, Cin, Cout, KS, s, 0, u64); } if (!v_ready) launch_wino_input(tile, x, v, N, H, W, Cin, KS, s, e.in_rbits_out); };
    auto post = [&]() {
        if (e.next_v && tile == 6 && KS == 3 && e.relu && e.bias && !e.addend && !e.mask && !e.dropout && !e.pool && !e.rbits_in &&
            launch_wino_out_in(mm, e.bias, e.next_v, e.rbits_out, N, H, W, Cout, s, m && m->fuse_out_in >= 2)) { if (e.fused_out) *e.fused_out = true; return; }
        launch_wino_output(tile, mm, e.bias, e.addend, e.mask, e.mask_scale, e.relu, (e.skip_y && e.pool) ? nullptr : y, N, H, W, Cout, e.dropout, e.keep, e.seed, e.stream_id, s, e.pool, e.pidx, KS, e.rbits_out, e.rbits_in); };
    // (bytes of the fused form: M read, the next conv's V written, the ReLU record)
    const double ob_fused = 4.0 * (2.0 * P * T * Cout + (e.rbits_out ? (double)N * H * W * Cout / 32 : 0.0));
    { ProfScope ps(m, "wino_transform", 0, (v_ready ? 0.0 : tb) + (u_cached ? 0.0 : (double)(KS * KS + P * nsub2 + (u64 ? P : 0)) * 4 * Cin * Cout)); pre(); }
    if (gemm_out64) {
        // one kernel from V to the pool: the scope keeps its name and flops (the roofline tables and pass_state.h's ledger stay comparable); bytes = V, the bank, pool and argmax bytes
        ProfScope ps(m, tag, 2.0 * P * T * Kg * Cout, 4.0 * P * (T * (double)Kg + (double)Kg * Cout) + (double)N * H * W * Cout * (1.0 + (e.pidx ? 0.25 : 0.0)), layer);
        m->gemm_out64_launches += 1;
        if (!launch_wino_gemm_out64(v, u64, e.bias, e.pool, e.pidx, N, H, W, s, m->gemm_out64_nt)) defer_error(FCN8S_ERR_HIP, "wino_gemm_out64_kernel could not be launched for %s (%d x %d x %d)", layer, N, H, W);
        return;
    }
    { ProfScope ps(m, tag, 2.0 * P * T * Kg * Cout, 4.0 * P * (T * (double)(Kg + Cout) + (double)Kg * Cout), layer); launch_igemm(a, P, s); }
    { ProfScope ps(m, "wino_transform", 0, ob); post(); if (e.fused_out && *e.fused_out && m && m->profile && !m->groups.empty()) { const int g = group_id(m, "wino_transform"); m->groups[g].bytes += ob_fused - ob; } }
}

// The direct form, where both directions end when no transform-domain path applies: the implicit-GEMM tile kernels or, for the 1x1 score heads, the
// skinny kernels.  `a` arrives with the caller's epilogue (bias, addend, mask, alpha, relu, mask_scale, dropout, keep_prob, stream_id).
static void conv_direct(fcn8s_model* m, const char* group, IgemmArgs a, const float* x, const float* w, float* y,
                        int N, int H, int W, int Cin, int Cout, int K, hipStream_t s, int real_cin, const char* layer)
{
    a.split = split_of(m);
    a.x = x; a.w = w; a.y = y;
    a.N = N; a.Ma = H; a.Mb = W; a.M = (long long)N * H * W;
    a.Hi = H; a.Wi = W; a.Cin = Cin; a.ldx = Cin;
    a.KW = K; a.in_scale = 1; a.tap_step = 1; a.tap_off = -(K - 1) / 2; a.Ktot = K * K * Cin;
    a.Ho = H; a.Wo = W; a.Cout = Cout; a.ldy = Cout;
    a.out_scale = 1; a.out_offy = 0; a.out_offx = 0; a.phases_x = 1; a.w_phase_stride = 0;
    a.seed = m ? m->seed : 0;
    const double rc = real_cin ? real_cin : Cin;
    const double flops = 2.0 * a.M * K * K * rc * Cout;
    const double bytes = 4.0 * (a.M * rc + (double)a.M * Cout + (double)K * K * rc * Cout);
    // 1x1 score heads: one skinny dimension (skinny.hip); everything else goes through the general tile kernels
    auto run = [&]() {
        if (K == 1 && !real_cin && !a.addend && !a.relu && !a.dropout) {
            if (Cout <= 32 && !a.mask && launch_head_fwd(x, w, a.bias, y, a.M, N, Cin, Cout, a.alpha, s, m ? m->d_wino_u : nullptr, m ? m->ufl : 0)) return;      // (the filter-bank scratch is idle between convolutions)
            if (Cin <= 32 && !a.bias && launch_head_dgrad(x, w, a.mask, a.mask_scale, y, a.M, Cout, Cin, a.alpha, s)) return;
        }
        launch_igemm(a, 1, s);
    };
    { ProfScope ps(m, group, flops, bytes, layer); run(); }
}

// SAME conv, forward.  Returns true if e.pool_out was written.
bool conv_fwd(fcn8s_model* m, const char* group, const float* x, const float* w, float* y,
              int N, int H, int W, int Cin, int Cout, int K, const FwdEpi& e, hipStream_t s, int real_cin = 0,
              const char* layer = nullptr)
{
    if (m && K == 7 && layer && !real_cin && e.alpha == 1.f && !e.pool_out && !e.relu_bits_out && m->fwd_train && fft6_on(m, N, H, W, Cin, Cout) &&
        conv_fft6_fwd(m, layer, x, w, y, N, H, W, Cin, Cout, e.bias, e.relu, e.dropout, e.keep, e.stream_id, s)) return false;
    if (m) m->pass.drop_backward_handoffs();
    const int tile = fwd_tile(route_opts(m), ConvShape{N, H, W, Cin, Cout, K});
    if (tile && !(K == 3 && e.dropout) && e.alpha == 1.f && !real_cin) {
        const bool v_ready = m->pass.fwd_v.take(layer);      // written by the previous conv's fused output transform
        m->pass.fwd_v.drop();                                // (another layer's V: a promise nobody collects any more)
        float* vbuf = m->d_wino_v;
        if (layer) { auto it = m->acts.find(std::string("wv:") + layer); if (it != m->acts.end()) vbuf = it->second.p; }      // training keeps V for the weight gradient
        WinoEpi we; we.bias = e.bias; we.relu = e.relu;
        we.dropout = e.dropout; we.keep = e.keep; we.seed = m->seed; we.stream_id = e.stream_id; we.pool = e.pool_out; we.pidx = e.pool_idx;
        we.rbits_out = e.relu_bits_out; we.skip_y = e.skip_y && e.pool_out;
        if (e.relu_bits_out && layer) m->pass.rbits_ok.insert(layer);
        if (e.in_relu_bits_out && e.in_layer && K == 3) { we.in_rbits_out = e.in_relu_bits_out; m->pass.rbits_ok.insert(e.in_layer); }
        bool fused_out = false;
        if (e.next_v && e.next_layer) { we.next_v = e.next_v; we.fused_out = &fused_out; }
        we.gemm_out_fused64 = e.gemm_out_fused64;
        conv_winograd(m, tile, K, true, x, w, y, m->d_wino_u, vbuf, m->d_wino_m, N, H, W, Cin, Cout, we, s, layer, v_ready);
        if (fused_out) { m->pass.fwd_v.give(e.next_layer); if (layer) m->pass.y_unwritten.insert(layer); }
        return e.pool_out != nullptr;
    }
    IgemmArgs a{}; a.bias = e.bias; a.alpha = e.alpha; a.relu = e.relu; a.mask_scale = 1.f; a.dropout = e.dropout; a.keep_prob = e.keep; a.stream_id = e.stream_id;
    conv_direct(m, group, a, x, w, y, N, H, W, Cin, Cout, K, s, real_cin, layer);
    return false;
}

// ---- the backward launchers: conv_dgrad and conv_wgrad are drivers over one function per route -------------------------------------------------------
// What every route receives.  fwd is the shape of the FORWARD convolution, the form conv_route.h speaks: the weight gradient reads X (fwd.Cin channels)
// and dZ (fwd.Cout); the data gradient reads dY (fwd.Cout channels) and writes dX (fwd.Cin).
struct BwdCall {
    fcn8s_model* m;                  // null: an op-level entry point without a model (only the direct forms run)
    hipStream_t s;
    const char* layer;               // null: a layer that no ledger entry and no kept bank knows (the score heads, the model-less entry points)
    const char* group;               // profile group of the direct form
    ConvShape fwd;
    bool promised = false;           // conv_wgrad: the layer was handed dM instead of dZ (pass.dm_prefilled)
};
// What a route reports.  taken: the launch sequence is finished, a deferred error that ends the pass included.  declined: the next candidate's turn.
enum class Route { taken, declined };
static bool bf16_train_step(const BwdCall& c) { return bf16_train_mode(c.m) && c.m->train_mode && c.layer; }

// FCN8S_PREC_BF16_TRAIN: the SAME convolution of the padded bf16 copy of dY with the flipped kernel, wt[ci][(flipped tap, co)] bf16, on
// conv_bf16_256_kernel; fp32 accumulate, fp32 epilogue (skip-path addend, the ReLU / dropout mask of the layer's input).  Where it declines past its
// condition it has grown d_wbf16 and, after a refused launch without column partials, run the weight relayout: conv_dgrad's guards come next.
static Route dgrad_bf16_train(const BwdCall& c, const float* dy, float* dx, const DgradEpi& e)
{
    fcn8s_model* m = c.m; hipStream_t s = c.s; const char* layer = c.layer;
    const int N = c.fwd.N, H = c.fwd.H, W = c.fwd.W, K = c.fwd.K, Cdy = c.fwd.Cout, Cdx = c.fwd.Cin;
    if (!(bf16_train_step(c) && e.w_fwd && e.alpha == 1.f && bf16_kernels_take(transposed(c.fwd)))) return Route::declined;
    const size_t wneed = (size_t)K * K * Cdy * Cdx;
    const bool ok = m->d_wbf16.grow(wneed * sizeof(unsigned short), s, &m->ws_allocs);
    unsigned short* dyb = ok ? dyb_for(m, layer, dy, N, H, W, Cdy, K, s) : nullptr;
    if (!dyb) return Route::declined;
    { ProfScope ps(m, "weight_relayout", 0, 6.0 * wneed); launch_w_to_bf16_flip_t(e.w_fwd, m->d_wbf16, K, Cdx, Cdy, s); }
    Bf16Conv256Args g{};
    g.xp = dyb; g.xp_ps = g16_ps(N, H, W, K); g.wt = m->d_wbf16; g.y = dx; g.N = N; g.H = H; g.W = W; g.Cin = Cdy; g.Cout = Cdx; g.K = K;
    g.addend = e.addend; g.mask = e.mask; g.mask_scale = e.mask_scale; g.any_shape = 1; g.guarded = 1; g.rows_bn = m->bf16_rows_bn;
    if (e.mask && K == 3 && e.mask_scale == 1.f) {          // the mask is the ReLU of this layer's input: its sign is in the layer's own bf16 input copy
        auto xi = m->xg16.find(layer);
        if (xi != m->xg16.end() && xi->second) { g.mask16 = xi->second + g16_off(bf16_guard_rows(3, W + 2), Cdx); g.mask16_ps = g16_ps(N, H, W, 3); }
    }
    // this gradient is the output gradient of layer e.yb_layer (same map).  If that layer's gradients read nothing else (dy_bf16_only, asked by the caller), this
    // kernel's epilogue writes its padded bf16 copy instead of the fp32 gradient, and takes its column sums, that layer's bias gradient, from the fp32 values
    const bool only16 = e.yb_layer && e.yb_only;
    if (only16) { g.yb = g16_for(m, m->dyg16, e.yb_layer, N, H, W, Cdx, e.yb_K, s); g.yb_pad = (e.yb_K - 1) / 2; g.yb_ps = g16_ps(N, H, W, e.yb_K); }
    long long prow = 0;
    if (g.yb) {
        prow = ((long long)N * (H + 2) * (W + 2) + conv_bf16_rows_bm(Cdx, g.rows_bn) - 1) / conv_bf16_rows_bm(Cdx, g.rows_bn);
        g.colpart = det_scratch(s, (size_t)prow * Cdx);
        if (g.colpart) g.y = nullptr; else prow = 0;
    }
    const double M = (double)N * H * W;
    bool done;
    { ProfScope ps(m, K == 1 ? "fc7_dgrad_bf16" : (K == 3 ? "conv3x3_dgrad_bf16" : "fc6_dgrad_bf16"), 2.0 * M * K * K * Cdy * Cdx,
                   (g.y ? 4.0 : 0.0) * M * Cdx + (g.yb ? 2.0 : 0.0) * M * Cdx + (g.mask16 ? 2.0 : (e.mask ? 4.0 : 0.0)) * M * Cdx + 2.0 * M * Cdy + 2.0 * wneed, layer);
      done = launch_conv_bf16_256(g, s); }
    if (done) {
        if (g.yb) m->pass.dyg16_filled.insert(e.yb_layer);
        if (g.colpart) {
            ProfScope ps(m, "colsum", 0, 4.0 * prow * Cdx);
            launch_colsum(g.colpart, Gp(m, std::string(e.yb_layer) + "/biases"), prow, Cdx, s);
            m->pass.db_taken.insert(e.yb_layer); m->pass.dy_bf16_only.insert(e.yb_layer);
        }
        return Route::taken;
    }
    if (g.colpart) { defer_error(FCN8S_ERR_SHAPE, "bf16_train: %s's data gradient was refused by the flat-position kernel", layer); return Route::taken; }      // (a refused launch: unreachable by rule, kept as the guard)
    return Route::declined;
}

// fc6 in the DFT domain (conv_fft6_dgrad), with the filter bank this step's forward pass kept and holds ready
static Route dgrad_fft6(const BwdCall& c, const float* dy, float* dx, const DgradEpi& e)
{
    fcn8s_model* m = c.m; const char* layer = c.layer;
    const int N = c.fwd.N, H = c.fwd.H, W = c.fwd.W, Cdy = c.fwd.Cout, Cdx = c.fwd.Cin;
    if (!(m && c.fwd.K == 7 && layer && e.alpha == 1.f && !e.addend && !e.mask && !e.relu_bits_in)) return Route::declined;
    auto kept = m->u_train.find(std::string(layer) + "#fft");
    if (!(m->pass.fft6_ready.holds(layer) && kept != m->u_train.end() && kept->second && fft6_on(m, N, H, W, Cdx, Cdy) && bt_gemm_ok(Cdy, Cdx))) return Route::declined;
    conv_fft6_dgrad(m, layer, dy, kept->second, dx, N, H, W, Cdy, Cdx, c.s);
    return Route::taken;
}

// 3x3, F(6x6): the adjoint of the forward Winograd algorithm, dV[xi] = dM[xi] U[xi]^T with the dM = A dY A^T the weight gradient just built (d_wino_m)
// and the FORWARD filter bank, then dx = overlap-added B dV B^T.  (e.w_fwd is [3,3,Cdx,Cdy].)
static Route dgrad_adjoint(const BwdCall& c, bool dm_ready, float* dx, const DgradEpi& e)
{
    fcn8s_model* m = c.m; hipStream_t s = c.s; const char* layer = c.layer;
    const int N = c.fwd.N, H = c.fwd.H, W = c.fwd.W, Cdy = c.fwd.Cout, Cdx = c.fwd.Cin;
    if (!(adjoint_dgrad(route_opts(m), c.fwd) && dm_ready && e.w_fwd && e.alpha == 1.f)) return Route::declined;
    const int P = 64;
    const long long T = wino_tiles(6, N, H, W);
    IgemmArgs a = position_gemm(m->d_wino_m, m->d_wino_u, m->d_wino_v, T, Cdy, Cdx); a.split = split_of(m);
    auto kept = m->u_train.find(std::string(layer) + "#6");
    if (kept != m->u_train.end() && kept->second && bt_gemm_ok(Cdy, Cdx)) {
        a.w = kept->second; a.bt = 1; a.ldw = Cdy;          // the forward bank U[xi][Cdx][Cdy], read transposed
    } else {
        // (a filter transform of the BACKWARD pass, into shared scratch: nothing a frozen model keeps, so no prof_derived count)
        ProfScope ps(m, "wino_transform", 0, (double)(9 + P) * 4 * Cdy * Cdx); launch_wino_filter(6, e.w_fwd, m->d_wino_u, Cdx, Cdy, 3, s, 1);
    }
    { ProfScope ps(m, "wino_gemm_dgrad", 2.0 * P * T * Cdy * Cdx, 4.0 * P * (T * (double)(Cdy + Cdx) + (double)Cdy * Cdx), layer); launch_igemm(a, P, s); }
    if (e.dm_out && e.dm_out_layer && e.relu_bits_in && !e.addend && e.mask_scale == 1.f) {
        // the consumer of this gradient is the previous conv's weight gradient in the Winograd domain: hand it dM, skip dZ
        ProfScope ps(m, "wino_transform", 0, 4.0 * ((double)N * H * W * Cdx / 32 + 2.0 * P * T * Cdx));
        launch_wino_dgrad_output_dout(m->d_wino_v, e.relu_bits_in, e.dm_out, N, H, W, Cdx, s);
        m->pass.dm_prefilled.give(e.dm_out_layer);
        return Route::taken;
    }
    { ProfScope ps(m, "wino_transform", 0, 4.0 * ((double)N * H * W * Cdx * (1.0 + (e.relu_bits_in ? 1.0 / 32 : (e.mask ? 1.0 : 0.0)) + (e.addend ? 1.0 : 0.0)) + (double)P * T * Cdx));
      launch_wino_dgrad_output(m->d_wino_v, e.addend, e.mask, e.mask_scale, e.relu_bits_in, dx, N, H, W, Cdx, s); }
    return Route::taken;
}

// fc6, F(4x4,4x4): the adjoint of the forward sub-filter Winograd algorithm (default widths: Cdy = 4096, Cdx = 512),
// dV[xi][t][sub * Cdx + c] = dM[xi][t][:] . U[xi][sub * Cdx + c][:] with the forward bank of this step read as a transposed B operand, then the
// overlap-add gather (winograd.hip).  No transform of dz, no second filter bank, no flipped copy.
static Route dgrad_fc6_adjoint(const BwdCall& c, bool dm_ready, float* dx, const DgradEpi& e)
{
    fcn8s_model* m = c.m; hipStream_t s = c.s; const char* layer = c.layer;
    const int N = c.fwd.N, H = c.fwd.H, W = c.fwd.W, Cdy = c.fwd.Cout, Cdx = c.fwd.Cin;
    if (!(c.fwd.K == 7 && fc6_wino_map(route_opts(m), H, W) && dm_ready && e.alpha == 1.f && !e.mask && !e.addend && bt_gemm_ok(Cdy, 4 * Cdx))) return Route::declined;
    auto kept = m->u_train.find(std::string(layer) + "#4");
    if (!(kept != m->u_train.end() && kept->second)) return Route::declined;
    const int P = 49, Ng = 4 * Cdx;
    const long long T = wino_tiles(4, N, H, W);
    IgemmArgs a = position_gemm(m->d_wino_m, kept->second, m->d_wino_v, T, Cdy, Ng); a.split = split_of(m);
    a.bt = 1; a.ldw = Cdy;
    { ProfScope ps(m, "wino_gemm_fc6_dgrad", 2.0 * P * T * Cdy * Ng, 4.0 * P * (T * (double)(Cdy + Ng) + (double)Cdy * Ng), layer); launch_igemm(a, P, s); }
    { ProfScope ps(m, "wino_transform", 0, 4.0 * ((double)N * H * W * Cdx + (double)P * T * Ng)); launch_wino_dgrad_output_sub44(m->d_wino_v, dx, N, H, W, Cdx, s); }
    return Route::taken;
}

// The forward algorithm on the flipped + transposed weights wt; v_ready: V = B^T dY B came with the weight gradient's dM (launch_wino_input_dout)
static Route dgrad_winograd(const BwdCall& c, bool v_ready, const float* dy, const float* wt, float* dx, const DgradEpi& e)
{
    fcn8s_model* m = c.m;
    const int tile = dgrad_tile(route_opts(m), c.fwd);
    if (!(tile && e.alpha == 1.f)) return Route::declined;
    WinoEpi we; we.addend = e.addend; we.mask = e.mask; we.mask_scale = e.mask_scale; we.seed = m->seed; we.rbits_in = e.relu_bits_in;
    conv_winograd(m, tile, c.fwd.K, false, dy, wt, dx, m->d_wino_u, m->d_wino_v, m->d_wino_m, c.fwd.N, c.fwd.H, c.fwd.W, c.fwd.Cout, c.fwd.Cin, we, c.s, c.layer, v_ready);
    return Route::taken;
}

// The direct form on wt: where every data gradient ends that no route above took
static void dgrad_direct(const BwdCall& c, const float* dy, const float* wt, float* dx, const DgradEpi& e)
{
    IgemmArgs a{}; a.addend = e.addend; a.mask = e.mask; a.alpha = e.alpha; a.mask_scale = e.mask_scale; a.keep_prob = 1.f;
    conv_direct(c.m, c.group, a, dy, wt, dx, c.fwd.N, c.fwd.H, c.fwd.W, c.fwd.Cout, c.fwd.Cin, c.fwd.K, c.s, 0, c.layer);
}

// Data gradient of a SAME conv: dy has Cdy channels, dx gets Cdx, `wt` holds (or, e.lazy_wt, is to hold) the flipped + transposed weights.
// The routes in order; the ledger's backward hand-offs are taken and dropped here, between the bf16 route and the rest.
void conv_dgrad(fcn8s_model* m, const char* group, const float* dy, const float* wt, float* dx,
                int N, int H, int W, int Cdy, int Cdx, int K, const DgradEpi& e, hipStream_t s, const char* layer = nullptr)
{
    const BwdCall c{m, s, layer, group, ConvShape{N, H, W, Cdx, Cdy, K}};
    if (dgrad_bf16_train(c, dy, dx, e) == Route::taken) return;
    // Unreachable by rule (dy_bf16_only / out_bf16_only / conv1_writes_bf16_only imply bf16_kernels_take of this launch: tests/test_bf16_route_host.py); kept as
    // the guards for an allocation failure and a refused launch.
    if (bf16_train_step(c) && m->pass.dy_bf16_only.count(layer)) {
        defer_error(FCN8S_ERR_SHAPE, "bf16_train: %s's data gradient could not run on the bf16 kernel and its fp32 output gradient was not kept (option \"bf16_acts\" = 0 keeps it)", layer); return;
    }
    if (bf16_train_step(c) && e.mask && m->pass.in_bf16_only.count(layer)) {
        defer_error(FCN8S_ERR_SHAPE, "bf16_train: %s's data gradient could not run on the bf16 kernel and its fp32 mask was not kept (option \"bf16_acts\" = 0 keeps it)", layer); return;
    }
    // what the layer's weight gradient left in the scratch for this call; anything left for another layer is void, this convolution overwrites it
    const bool dm_ready = m && m->pass.dm.take(layer), v_ready = m && m->pass.dgrad_v.take(layer);
    if (m) m->pass.drop_backward_handoffs();
    if (dgrad_fft6(c, dy, dx, e) == Route::taken) return;
    if (dgrad_adjoint(c, dm_ready, dx, e) == Route::taken) return;
    if (dgrad_fc6_adjoint(c, dm_ready, dx, e) == Route::taken) return;
    if (e.lazy_wt && e.w_fwd) {          // (the routes above read w_fwd itself)
        ProfScope ps(m, "weight_relayout", 0, 8.0 * K * K * Cdy * Cdx); launch_flip_transpose(e.w_fwd, const_cast<float*>(wt), K * K, Cdx, Cdy, s);
    }
    if (dgrad_winograd(c, v_ready, dy, wt, dx, e) == Route::taken) return;
    dgrad_direct(c, dy, wt, dx, e);
}

// transposed conv forward (k = 2s) as s*s phase-specific 2x2 convs; wp = phase-packed weights
void tconv_fwd(fcn8s_model* m, const float* x, const float* wp, const float* bias, const float* addend,
               float* y, int N, int Hi, int Wi, int C, int K, int S, hipStream_t s)
{
    IgemmArgs a{}; a.split = split_of(m);
    a.x = x; a.w = wp; a.bias = bias; a.addend = addend; a.mask = nullptr; a.y = y;
    a.N = N; a.Ma = Hi + 1; a.Mb = Wi + 1; a.M = (long long)N * a.Ma * a.Mb;
    a.Hi = Hi; a.Wi = Wi; a.Cin = C; a.ldx = C;
    a.KW = 2; a.in_scale = 1; a.tap_step = -1; a.tap_off = 0; a.Ktot = 4 * C;
    a.Ho = Hi * S; a.Wo = Wi * S; a.Cout = C; a.ldy = C;
    a.out_scale = S; a.out_offy = -(K - S) / 2; a.out_offx = -(K - S) / 2;
    a.phases_x = S; a.w_phase_stride = 4LL * C * C;
    a.alpha = 1.f; a.relu = 0; a.mask_scale = 1.f; a.dropout = 0;
    const double opix = (double)N * Hi * S * Wi * S;
    ProfScope ps(m, "tconv_fwd", 2.0 * opix * 4 * C * C, 4.0 * (opix * C * (addend ? 2 : 1) + (double)N * Hi * Wi * C)); launch_igemm(a, S * S, s);
}

// data gradient of the transposed conv = stride-S conv of dy with the natural [kh,kw,Cout,Cin] kernel
void tconv_dgrad(fcn8s_model* m, const float* dy, const float* w, float* dx, int N, int Hi, int Wi, int C,
                 int K, int S, hipStream_t s)
{
    IgemmArgs a{}; a.split = split_of(m);
    a.x = dy; a.w = w; a.y = dx;
    a.N = N; a.Ma = Hi; a.Mb = Wi; a.M = (long long)N * Hi * Wi;
    a.Hi = Hi * S; a.Wi = Wi * S; a.Cin = C; a.ldx = C;
    a.KW = K; a.in_scale = S; a.tap_step = 1; a.tap_off = -(K - S) / 2; a.Ktot = K * K * C;
    a.Ho = Hi; a.Wo = Wi; a.Cout = C; a.ldy = C;
    a.out_scale = 1; a.phases_x = 1; a.alpha = 1.f; a.mask_scale = 1.f;
    const double flops = 2.0 * a.M * K * K * C * C;
    ProfScope ps(m, "tconv_dgrad", flops, 4.0 * ((double)N * Hi * S * Wi * S * C + (double)a.M * C)); launch_igemm(a, 1, s);
}

static void broken_promise(const BwdCall& c) { defer_error(FCN8S_ERR_STATE, "%s was handed dM instead of dZ but does not take the Winograd-domain path", c.layer); }

// Option keep_output_gradients: the layer's fp32 dY, copied before any route consumes it
static void keep_output_gradient(const BwdCall& c, const float* dz, const unsigned char* pool_idx)
{
    fcn8s_model* m = c.m; const char* layer = c.layer;
    if (!(m && m->keep_dy && layer)) return;
    // (dz holds the layer's fp32 dY unless it was handed over in another form: dM from the next layer's data gradient, d(pool) with routing bytes, a bf16 copy only)
    fcn8s_model::KeptDy& k = m->kept_dy[layer];
    const size_t n = (size_t)c.fwd.N * c.fwd.H * c.fwd.W * c.fwd.Cout;
    k.n = 0;
    if (!(c.promised || pool_idx || m->pass.dy_bf16_only.count(layer) || m->pass.dz_unwritten.count(layer))) {
        if (k.p.grow(n * sizeof(float), c.s)) { k.n = n; hipMemcpyAsync(k.p, dz, n * sizeof(float), hipMemcpyDeviceToDevice, c.s); }
        else defer_error(FCN8S_ERR_OOM, "keep_output_gradients: %s's copy cannot be allocated", layer);
    }
}

// FCN8S_PREC_BF16_TRAIN: dW[tap] = (padded bf16 input, moved by the tap)^T (padded bf16 dY), fp32 accumulate (gemm_bf16.hip: wgrad_bf16_kernel);
// the bias gradient is the exact fp32 column sum of dY.  Declines without the layer's input copy or its dY copy, and after a refused launch that
// has not taken the bias gradient: conv_wgrad's guard comes next.
static Route wgrad_bf16_train(const BwdCall& c, const float* dz, float* dw, float* db, float alpha, int real_cin)
{
    fcn8s_model* m = c.m; hipStream_t s = c.s; const char* layer = c.layer;
    const int N = c.fwd.N, H = c.fwd.H, W = c.fwd.W, Cin = c.fwd.Cin, Cout = c.fwd.Cout, K = c.fwd.K;
    if (!(bf16_train_step(c) && !real_cin && alpha == 1.f && bf16_kernels_take(c.fwd))) return Route::declined;
    auto it = m->xg16.find(layer);
    if (!(it != m->xg16.end() && it->second)) return Route::declined;
    const long long P = (long long)N * H * W;
    const int pad = (K - 1) / 2, Wp_ = W + 2 * pad;
    const long long G = bf16_guard_rows(K, Wp_), R = (long long)N * (H + 2 * pad) * Wp_;
    bool db_done = false;
    unsigned short* dyb = dyb_for(m, layer, dz, N, H, W, Cout, K, s, db, &db_done);
    if (m->pass.db_taken.count(layer)) db_done = true;          // (the kernel that wrote this layer's dY copy added the bias gradient too)
    if (!dyb) return Route::declined;
    Bf16WgradArgs g{};
    g.A = it->second + g16_off(G, Cin); g.B = dyb; g.C = dw; g.R = R; g.Ci = Cin; g.Cj = Cout; g.K = K; g.Wp = Wp_; g.a_ps = g.b_ps = g16_ps(N, H, W, K);
    bool done;
    { ProfScope ps(m, K == 1 ? "fc7_wgrad_bf16" : (K == 3 ? "conv3x3_wgrad_bf16" : "fc6_wgrad_bf16"), 2.0 * P * K * K * (double)Cin * Cout, 2.0 * K * K * R * (Cin + Cout) + 4.0 * K * K * Cin * Cout, layer);
      done = launch_wgrad_bf16(g, s); }
    if (done) {
        if (db && !db_done) { ProfScope ps(m, "colsum", 0, 4.0 * P * Cout); launch_colsum(dz, db, P, Cout, s); }
        return Route::taken;
    }
    if (db_done) { defer_error(FCN8S_ERR_SHAPE, "bf16_train: %s's weight-gradient launch refused its shape after the bias gradient was taken", layer); return Route::taken; }      // (a refused launch: unreachable by rule, kept as the guard)
    return Route::declined;
}

// fc6 in the DFT domain (conv_fft6_wgrad), on the Xf the forward pass kept: taking pass.fft6_xf, the last operand of the condition, is what decides
static Route wgrad_fft6(const BwdCall& c, const float* dz, float* dw, float* db, float alpha, int real_cin)
{
    fcn8s_model* m = c.m; const char* layer = c.layer;
    if (!(m && c.fwd.K == 7 && alpha == 1.f && !real_cin && m->train_mode && m->pass.fft6_xf.take(layer))) return Route::declined;
    if (c.promised) broken_promise(c);
    m->pass.drop_backward_handoffs();
    conv_fft6_wgrad(m, layer, m->acts[std::string("wv:") + layer].p, dz, dw, db, c.fwd.N, c.fwd.H, c.fwd.W, c.fwd.Cin, c.fwd.Cout, c.s);
    return Route::taken;
}

// 3x3 and fc6 in the Winograd domain, on the V the forward pass kept ("wv:<layer>"): dM = A dz A^T into d_wino_m, dU[xi] = V[xi]^T dM[xi], dW = G^T dU G.
// The layer's data gradient follows, and what this route leaves for it in the scratch it gives to the ledger: dM (pass.dm) for the adjoint routes,
// V = B^T dz B (pass.dgrad_v) for the forward-type one.
static Route wgrad_winograd(const BwdCall& c, const float* dz, float* dw, float* db, float alpha, int real_cin, const unsigned char* pool_idx)
{
    fcn8s_model* m = c.m; hipStream_t s = c.s; const char* layer = c.layer;
    const int N = c.fwd.N, H = c.fwd.H, W = c.fwd.W, Cin = c.fwd.Cin, Cout = c.fwd.Cout, K = c.fwd.K;
    if (!(m && (K == 3 || K == 7) && layer && alpha == 1.f && !real_cin && m->train_mode)) return Route::declined;
    auto it = m->acts.find(std::string("wv:") + layer);
    // (fc6's slot also exists on maps that only the DFT tiles cover, e.g. 10x13: no F(4x4,4x4) tile there)
    if (!(it != m->acts.end() && m->d_wino_m && (K == 3 || wino_tile_for(m, H, W, 7) == 4))) return Route::declined;
    // fuse_dgrad_input: the data gradient runs through Winograd and its input transform V = B^T dz B can be written into d_wino_v by the same
    // kernel that writes dM (one read of dz); adj_bytes: it is the adjoint one, which consumes dM itself
    const RouteOpts ro = route_opts(m);
    const bool fuse_dgrad_input = dgrad_input_fused(ro, c.fwd), adj_bytes = adjoint_dgrad(ro, c.fwd);
    const int tile = wino_tile_for(m, H, W, K), NP = wino_alpha(tile, K) * wino_alpha(tile, K);
    const long long T = wino_tiles(tile, N, H, W);
    const int Kg = wino_nsub(K) * wino_nsub(K) * Cin;           // rows of V / dU: [sub-filter][channel]
    WgradArgs g = position_wgrad(it->second.p, m->d_wino_m, m->d_wino_u, T, Kg, Cout, NP); g.split = split_of(m);
    bool fused = false, dm_ready = false;
    const bool prefilled = c.promised && adj_bytes && !pool_idx;      // dM already in d_wino_m (wino_dgrad_output_dout_kernel)
    if (c.promised && !prefilled) broken_promise(c);
    if (prefilled) dm_ready = true;
    else {
        { ProfScope ps(m, "wino_transform", 0, 4.0 * ((double)N * H * W * Cout * (pool_idx ? 0.3125 : 1.0) + ((fuse_dgrad_input && !adj_bytes) ? 2.0 : 1.0) * NP * T * Cout));
          // pool_idx: dz is d(pool) [N,H/2,W/2,Cout]; the max-pool backward happens inside the transform (the caller checked eligibility)
          // adjoint data gradient (tile 6): it consumes dM itself, no second transform of dz
          if (adj_bytes) { launch_wino_dout(6, dz, m->d_wino_m, N, H, W, Cout, s, 3, pool_idx); dm_ready = true; }
          else {
              if (fuse_dgrad_input) fused = launch_wino_input_dout(tile, dz, m->d_wino_v, m->d_wino_m, N, H, W, Cout, s, pool_idx);
              if (!fused) launch_wino_dout(tile, dz, m->d_wino_m, N, H, W, Cout, s, K);
          } }
        // fc6: the non-fused transform above left dM = A dz A^T in d_wino_m; its adjoint data gradient (dgrad_fc6_adjoint) consumes it
        // (not when this step's forward ran through the DFT tiles: a kept F(4x4,4x4) bank would be stale)
        if (K == 7 && tile == 4 && !fused && Cin % 2 == 0 && bt_gemm_ok(Cout, 4 * Cin) && m->u_train.count(std::string(layer) + "#4") && !m->pass.fft6_ready.holds(layer)) dm_ready = true;
    }
    m->pass.drop_backward_handoffs();
    if (fused) m->pass.dgrad_v.give(layer);
    if (dm_ready) m->pass.dm.give(layer);
    { ProfScope ps(m, K == 7 ? "wino_gemm_fc6_wgrad" : "wino_gemm_wgrad", 2.0 * NP * T * Kg * Cout, 4.0 * NP * (T * (double)(Kg + Cout) + (double)Kg * Cout), layer); launch_wgrad(g, s); }
    { ProfScope ps(m, "wino_transform", 0, 4.0 * (9.0 + NP) * Cin * Cout + 4.0 * N * H * W * Cout * (tile >= 4 ? 1.0 / (tile * tile) : 1.0));
      launch_wino_dfilter(tile, m->d_wino_u, dw, Cin, Cout, K, s);
      // bias gradient = sum of dz over all pixels.  dM[(1,1)] = sum_kl A^T(k,1) dz[k][l] A^T(l,1) and column 1 of A^T is all ones:
      // the slab of position (1,1) holds the per-tile sums -- 16x fewer bytes than dz, and dz need not exist
      if (db) {
          if (tile >= 4) launch_colsum(m->d_wino_m + (wino_alpha(tile, K) + 1) * wino_slab(T, Cout), db, T, Cout, s);
          else launch_colsum(dz, db, (long long)N * H * W, Cout, s);
      } }
    return Route::taken;
}

// The direct forms, where every weight gradient ends that no route above took: the skinny kernel of the score heads, the per-tap kernels, conv1_1's own,
// the general one
static void wgrad_direct(const BwdCall& c, const float* x, const float* dz, float* dw, float* db, float alpha, int real_cin)
{
    fcn8s_model* m = c.m; hipStream_t s = c.s;
    const int N = c.fwd.N, H = c.fwd.H, W = c.fwd.W, Cin = c.fwd.Cin, Cout = c.fwd.Cout, K = c.fwd.K;
    WgradArgs a{}; a.split = split_of(m);
    a.A = x; a.B = dz; a.C = dw;
    a.N = N; a.Pa = H; a.Pb = W; a.P = (long long)N * H * W;
    a.Ha = H; a.Wa = W; a.Adim = Cin; a.lda = Cin; a.Areal = real_cin ? real_cin : Cin;
    a.Bdim = Cout; a.ldb = Cout;
    a.KW = K; a.a_scale = 1; a.tap_off = -(K - 1) / 2; a.ntaps = K * K;
    a.ldc = Cout; a.alpha = alpha; a.colsum = db;
    const double rc = a.Areal;
    const double flops = 2.0 * a.P * K * K * rc * Cout;
    const double bytes = 4.0 * (a.P * rc + (double)a.P * Cout + (double)K * K * rc * Cout);
    const bool taps = (K == 3 || K == 7) && alpha == 1.f && !real_cin;
    const bool first = K == 3 && alpha == 1.f && real_cin == 3 && Cin == 4;
    auto run = [&]() {
        if (K == 1 && !real_cin && Cout <= 32 && launch_head_wgrad(x, dz, dw, a.P, Cin, Cout, alpha, s)) {
            if (db) launch_colsum(dz, db, a.P, Cout, s);
            return;
        }
        if (taps && launch_wgrad_taps(x, dz, dw, db, N, H, W, Cin, Cout, K, s)) return;
        if (first && launch_conv1_wgrad(x, dz, dw, db, N, H, W, Cout, m->conv1_wgrad_mfma, s)) return;
        launch_wgrad(a, s);
    };
    { ProfScope ps(m, c.group, flops, bytes, c.layer); run(); }
}

// Weight (and bias) gradient of a SAME conv.  The routes in order; whether the layer was handed dM instead of dZ (pass.dm_prefilled, from the data
// gradient of the layer after it: backward_blocks) is taken here and travels in the call, and a promise no Winograd-domain route can keep is reported
// before the DFT route runs, inside the Winograd route, and before the direct one.
void conv_wgrad(fcn8s_model* m, const char* group, const float* x, const float* dz, float* dw, float* db,
                int N, int H, int W, int Cin, int Cout, int K, float alpha, hipStream_t s, int real_cin = 0,
                const char* layer = nullptr, const unsigned char* pool_idx = nullptr)
{
    BwdCall c{m, s, layer, group, ConvShape{N, H, W, Cin, Cout, K}};
    c.promised = m && m->pass.dm_prefilled.take(layer);      // dz then holds nothing
    if (m) m->pass.dm_prefilled.drop();      // (a promise to another layer: d_wino_m is about to be rewritten)
    keep_output_gradient(c, dz, pool_idx);
    if (wgrad_bf16_train(c, dz, dw, db, alpha, real_cin) == Route::taken) return;
    // Unreachable by rule (whoever put the layer into either set asked bf16_kernels_take of this shape); kept as the guard for an allocation failure and a refused launch.
    if (bf16_train_step(c) && (m->pass.in_bf16_only.count(layer) || m->pass.dy_bf16_only.count(layer))) {
        defer_error(FCN8S_ERR_SHAPE, "bf16_train: %s's weight gradient could not run on the bf16 kernel and its fp32 input was not kept (option \"bf16_acts\" = 0 keeps it)", layer); return;
    }
    if (wgrad_fft6(c, dz, dw, db, alpha, real_cin) == Route::taken) return;
    if (wgrad_winograd(c, dz, dw, db, alpha, real_cin, pool_idx) == Route::taken) return;
    if (c.promised) broken_promise(c);
    wgrad_direct(c, x, dz, dw, db, alpha, real_cin);
}

void tconv_wgrad(fcn8s_model* m, const float* x, const float* dy, float* dw, int N, int Hi, int Wi, int C,
                 int K, int S, hipStream_t s)
{
    WgradArgs a{}; a.split = split_of(m);
    a.A = dy; a.B = x; a.C = dw;
    a.N = N; a.Pa = Hi; a.Pb = Wi; a.P = (long long)N * Hi * Wi;
    a.Ha = Hi * S; a.Wa = Wi * S; a.Adim = C; a.lda = C; a.Areal = C;
    a.Bdim = C; a.ldb = C;
    a.KW = K; a.a_scale = S; a.tap_off = -(K - S) / 2; a.ntaps = K * K;
    a.ldc = C; a.alpha = 1.f; a.colsum = nullptr;
    auto run = [&]() { if (!launch_tconv_wgrad(x, dy, dw, N, Hi, Wi, C, K, S, s)) launch_wgrad(a, s); };
    ProfScope ps(m, "tconv_wgrad", 2.0 * a.P * K * K * C * C, 4.0 * ((double)N * Hi * S * Wi * S * C + (double)a.P * C)); run();
}

// ---- workspace --------------------------------------------------------------------
// The arena's layout for one (N, H, W): named items at 256-byte aligned offsets, then the staged images / labels, predictions and loss partials.
struct WsItem { std::string name; size_t n; int h, w, c; float** extra; };
struct WsPlan { std::vector<WsItem> items; std::vector<Layer> layers; std::vector<size_t> offs; size_t o_img = 0, o_lab = 0, o_pred = 0, o_part = 0, bytes = 0; };
int check_shape(fcn8s_model* m, int N, int H, int W)
{
    if (N <= 0) return fail(m, FCN8S_ERR_SHAPE, "batch size must be positive");
    if (H <= 0 || W <= 0 || H % 32 || W % 32)
        return fail(m, FCN8S_ERR_SHAPE, "image height and width must be positive multiples of 32 (five 2x2 pools, then x2, x2, x8 upsampling must line up with the skip connections)");
    return FCN8S_OK;
}
// The table's names, shapes and parameter offsets for an H x W image: the one place that spells a layer's name.
static void fill_layer_table(const fcn8s_model* m, int H, int W, std::vector<Layer>& layers)
{
    layers.assign(15, Layer{});
    int k = 0, cin = 4;
    for (int b = 0; b < 7; ++b) {
        const int nconv = b < 5 ? kConvsPerBlock[b] : 1, shift = std::min(b, 5);
        for (int i = 1; i <= nconv; ++i, ++k) {
            Layer& L = layers[k];
            if (b < 5) snprintf(L.name, sizeof L.name, "conv%d_%d", b + 1, i); else snprintf(L.name, sizeof L.name, "fc%d", b + 1);
            if (b < 5) { snprintf(L.pool_name, sizeof L.pool_name, "pool%d", b + 1); snprintf(L.pool_in, sizeof L.pool_in, "pool%din", b + 1); }
            L.block = b + 1; L.pos = i; L.nconv = nconv;
            L.h = H >> shift; L.w = W >> shift; L.cin = cin; L.cout = m->widths[b]; L.K = b < 5 ? 3 : (b == 5 ? m->fc6k : 1); L.real_cin = k == 0 ? 3 : 0;
            L.prev = k - 1; L.next = k + 1 < 15 ? k + 1 : -1;
            L.w_off = P(m, std::string(L.name) + (b < 5 ? "/filter" : "/weights")).offset; L.b_off = P(m, std::string(L.name) + "/biases").offset;
            L.i_y = L.i_rb = L.i_wv = L.i_pool = L.i_pidx = -1;
            cin = L.cout;
        }
    }
}
static Layer* in_block_next(std::vector<Layer>& v, const Layer& L) { return L.pos < L.nconv ? &v[L.next] : nullptr; }
static Layer* in_block_prev(std::vector<Layer>& v, const Layer& L) { return L.pos > 1 ? &v[L.prev] : nullptr; }
static Layer* find_layer(fcn8s_model* m, const char* name) { for (Layer& L : m->layers) if (!strcmp(L.name, name)) return &L; return nullptr; }

// (sets m->plan_N = N: the batch size the per-layer Winograd tiles are chosen for, wino_tile_for, from here until the next re-plan.  The layer
//  table goes into the plan, pl.layers; carve_workspace makes it the model's)
void plan_workspace(fcn8s_model* m, int N, int H, int W, WsPlan& pl)
{
    m->plan_N = N;
    const int C = m->C;
    using Item = WsItem;
    std::vector<Item>& items = pl.items;
    items.clear(); pl.offs.clear();
    auto add = [&](const std::string& nm, int h, int w, int c, float** extra = nullptr) {
        items.push_back({nm, (size_t)N * h * w * c, h, w, c, extra});
        return (int)items.size() - 1;
    };
    auto add_raw = [&](const std::string& nm, size_t n, float** extra = nullptr) { items.push_back({nm, n, 0, 0, 0, extra}); return (int)items.size() - 1; };
    // The plan is what makes the shared scratch, so its rules run with scratch = true: every fact that asks for the scratch implies a layer that
    // scratch_channels() sizes it for (tests/test_conv_route_host.py: "fits the scratch").
    RouteOpts ro = route_opts(m); ro.scratch = true;
    auto slab_floats = [&](int hh, int ww, int c, int K) -> size_t {      // P slabs of wino_slab(T, nsub^2 c) floats
        const int tile = wino_tile_for(ro, hh, ww, K);
        if (!tile) return 0;
        const int al = wino_alpha(tile, K), ns = wino_nsub(K);
        return (size_t)al * al * (size_t)wino_slab(wino_tiles(tile, N, hh, ww), ns * ns * c);
    };
    // one walk over the layers: each layer's route facts, and the sizes that follow from them
    fill_layer_table(m, H, W, pl.layers);
    size_t vmax = 0, gmax = 0;         // Winograd scratch: the largest [P][T][C] tensor any layer needs (V and M of the forward and of the data-gradient conv); the largest gradient tensor
    std::vector<size_t> n_rb(pl.layers.size(), 0), n_wv(pl.layers.size(), 0);
    for (size_t k = 0; k < pl.layers.size(); ++k) {
        Layer& L = pl.layers[k];
        gmax = std::max(gmax, (size_t)N * L.h * L.w * L.cout);
        if (L.block > 5) continue;          // (fc6's routes are conv_fwd's / conv_wgrad's own; its scratch: fc6_scratch_floats below)
        const ConvShape sh = L.shape(N);
        const Layer* nx = in_block_next(pl.layers, L);
        L.tile = wino_tile_for(ro, L.h, L.w, 3);
        L.rb_writer = nx ? relu_record_writer(ro, sh, nx->shape(N), L.first()) : RbWriter::none;      // (only a conv that feeds another conv has a record)
        L.out_in_next = nx && out_in_fused(ro, sh, nx->shape(N));
        L.conv1_in_next = L.first() && nx && nx->last_of_block() && conv1_in_next_transform(ro, sh, nx->shape(N));
        L.dm_from_next = nx && dm_from_next(ro, sh);
        L.pool_in_transform = L.last_of_block() && pool_in_transform(ro, sh, in_block_prev(pl.layers, L) != nullptr);
        L.gemm_out_fused64 = L.last_of_block() && gemm_out_fused64(ro, sh, in_block_prev(pl.layers, L) != nullptr, L.block == 1);
        if (L.rb_writer != RbWriter::none) n_rb[k] = wino_rbits_words(L.tile, N, L.h, L.w, L.cout);
        if (keeps_v(ro, sh)) n_wv[k] = slab_floats(L.h, L.w, L.cin, 3);          // the forward pass keeps each Winograd layer's transformed input for the weight gradient
        if (const int c = scratch_channels(ro, sh)) vmax = std::max(vmax, slab_floats(L.h, L.w, c, 3));
    }
    // the arena's items, in its order
    add("x0", H, W, 4);
    for (Layer& L : pl.layers) {
        if (L.block > 5) break;
        L.i_y = add(L.name, L.h, L.w, L.cout);
        if (L.last_of_block()) { const int ip = add(L.pool_name, L.h / 2, L.w / 2, L.cout); for (int k = 0; k < L.nconv; ++k) (&L - k)->i_pool = ip; }
    }
    const int h5 = H / 32, w5 = W / 32, h4 = H / 16, w4 = W / 16, h3 = H / 8, w3 = W / 8;
    // ReLU bit masks of the convs whose output is another conv's input (read back by that conv's data gradient)
    for (size_t k = 0; k < pl.layers.size(); ++k) if (n_rb[k]) pl.layers[k].i_rb = add_raw(std::string("rb:") + pl.layers[k].name, n_rb[k]);
    for (Layer& L : pl.layers)      // argmax bytes of pool_b (one per pooled element), see launch_wino_output
        if (L.block <= 5 && L.last_of_block()) {
            const int ip = add_raw("pidx" + std::to_string(L.block), ((size_t)N * (L.h / 2) * (L.w / 2) * (size_t)L.cout + 3) / 4);
            for (int k = 0; k < L.nconv; ++k) (&L - k)->i_pidx = ip;
        }
    for (Layer& L : pl.layers) if (L.block > 5) L.i_y = add(L.name, L.h, L.w, L.cout);      // fc6, fc7
    add("s7", h5, w5, C); add("p4", h4, w4, C); add("p3", h3, w3, C);
    add("a4", h4, w4, C); add("a3", h3, w3, C); add("logits", H, W, C);
    add("dlogits", H, W, C, &m->dlogits);
    if (m->tconv_gemm) {
        const size_t rows = (size_t)N * (H / 8 + 1) * (W / 8 + 1);
        add_raw("logits_b", rows * 64 * C, &m->logits_b);
        add_raw("dlogits_b", rows * 64 * C, &m->dlogits_b);
        add_raw("tg_A", rows * m->tg_kp, &m->tg_A);
        add_raw("tg_dA", rows * m->tg_kp, &m->tg_dA);
    }
    add("da3", h3, w3, C, &m->da3); add("da4", h4, w4, C, &m->da4); add("ds7", h5, w5, C, &m->ds7);
    add("gskip3", h3, w3, m->widths[2], &m->gskip3); add("gskip4", h4, w4, m->widths[3], &m->gskip4);
    add_raw("gbuf0", gmax, &m->gbuf[0]);
    add_raw("gbuf1", gmax, &m->gbuf[1]);
    items.push_back({"softmax", (size_t)N * H * W * C, H, W, C, &m->d_softmax});
    {
        const Fc6Scratch f6 = fc6_scratch_floats(m, N, h5, w5, m->widths[4], m->widths[5]);
        vmax = std::max(vmax, f6.v_wino);      // V: P * T * nsub^2 * c5;  M: P * T * c6
        size_t mmax = vmax;
        vmax = std::max(vmax, f6.v_fft);       // fc6 through DFT tiles
        mmax = std::max(mmax, f6.m_fft);
        if (vmax) { add_raw("wino_v", vmax, &m->d_wino_v); add_raw("wino_m", mmax, &m->d_wino_m); }
        for (size_t k = 0; k < pl.layers.size(); ++k) if (n_wv[k]) pl.layers[k].i_wv = add_raw(std::string("wv:") + pl.layers[k].name, n_wv[k]);
        // fc6's slot holds V of F(4x4,4x4) or, when the weight gradient runs in the DFT domain, Xf: sized for either
        if (fc6_keeps_v(ro) && f6.wv) pl.layers[13].i_wv = add_raw("wv:fc6", f6.wv);
    }

    size_t bytes = 0;
    for (auto& it : items) { pl.offs.push_back(bytes); bytes = align_up(bytes + it.n * sizeof(float), 256); }
    const size_t npix = (size_t)N * H * W;
    pl.o_img = bytes;  bytes = align_up(bytes + npix * 3 * sizeof(float), 256);
    pl.o_lab = bytes;  bytes = align_up(bytes + npix, 256);
    pl.o_pred = bytes; bytes = align_up(bytes + npix * sizeof(long long), 256);
    pl.o_part = bytes; bytes = align_up(bytes + 4096 * sizeof(double), 256);
    pl.bytes = bytes;
}
// point the model's tensors into the arena (>= pl.bytes) at the plan's offsets
void carve_workspace(fcn8s_model* m, int N, int H, int W, const WsPlan& pl)
{
    m->acts.clear();
    m->have_forward = m->have_loss = false;
    m->pm = PixMap{m->tconv_gemm ? 1 : 0, H, W, H / 8 + 1, W / 8 + 1, 8};
    m->logits_b = m->dlogits_b = m->tg_A = m->tg_dA = nullptr;
    m->d_wino_v = m->d_wino_m = nullptr;
    for (size_t i = 0; i < pl.items.size(); ++i) {
        float* p = (float*)(m->arena + pl.offs[i]);
        if (pl.items[i].extra) *pl.items[i].extra = p;
        Act a; a.p = p; a.n = pl.items[i].n; a.H = pl.items[i].h; a.W = pl.items[i].w; a.C = pl.items[i].c;
        m->acts[pl.items[i].name] = a;
    }
    m->layers = pl.layers;      // (the plan's own copy: fcn8s_predict_tta plans shapes it only wants the size of)
    auto view = [&](int i) { return i < 0 ? nullptr : (float*)(m->arena + pl.offs[i]); };
    for (Layer& L : m->layers) { L.y = view(L.i_y); L.wv = view(L.i_wv); L.pool = view(L.i_pool); L.rb = (unsigned*)view(L.i_rb); L.pidx = (unsigned char*)view(L.i_pidx); }
    m->d_images = m->arena + pl.o_img; m->d_labels = (uint8_t*)(m->arena + pl.o_lab);
    m->d_pred = (long long*)(m->arena + pl.o_pred); m->d_partials = (double*)(m->arena + pl.o_part);
    m->N = N; m->H = H; m->W = W;
}
// ---- buffer lifetimes ---------------------------------------------------------------
// What the model allocates lazily dies with one of four things; each is one function, called from every place that means it.  Each waits for
// the stream before it frees (a kernel in flight may still read the buffer).  fcn8s_destroy needs none of them: the members free themselves.
//
// The arena (another plan: another shape, precision class or layout option) and every view into it.
void drop_arena(fcn8s_model* m)
{
    if (m->arena) hipStreamSynchronize(m->stream);
    m->arena.reset();
    m->N = m->H = m->W = 0; m->acts.clear();
    for (Layer& L : m->layers) { L.y = L.wv = L.pool = nullptr; L.rb = nullptr; L.pidx = nullptr; }
    m->have_forward = m->have_loss = false;
}
// The per-layer padded copies whose geometry is the workspace's shape: xbf16 (bf16 forward modes), xg16 / dyg16 (bf16_train), q8 (fp8_infer).
// keep_regrowable (fcn8s_predict_tta's re-plans, ensure_workspace_at_least): a pass shape comes back many times per call, so the copies that
// can serve another shape in place stay -- xg16 / dyg16 are only marked stale (g16_for zeroes the new border, and regrows if too small),
// q8 re-borders itself on a geometry change (q8_for) -- and only xbf16, which is sized once and never checked again, is dropped.
void drop_shape_copies(fcn8s_model* m, bool keep_regrowable = false)
{
    if (!m->xbf16.empty() || (!keep_regrowable && !(m->xg16.empty() && m->dyg16.empty() && m->q8.empty()))) hipStreamSynchronize(m->stream);
    m->xbf16.clear();
    m->pass.forget_shape_copies(keep_regrowable);
    if (keep_regrowable) {
        for (auto& kv : m->xg16) m->g16_stale.insert("x:" + kv.first);
        for (auto& kv : m->dyg16) m->g16_stale.insert("d:" + kv.first);
        return;
    }
    m->xg16.clear(); m->dyg16.clear(); m->g16_stale.clear();
    m->q8.clear();
}
// The banks made from one version of the parameters and kept while the model is frozen, of three kinds: the Winograd filter banks (u_cache)
// and the bf16 kernels (wbf16_cache), with the record of which of them fcn8s_predict_tta left stale, and fp8_infer's e4m3 weight banks, which
// keep their storage (w8) and lose only their validity (w8_valid: the next pass refills them).  Every occasion drops all three --
// fcn8s_freeze_params, fcn8s_set_precision, a mismatch found by forward()'s fingerprint guard -- but one: fcn8s_set_option passes keep_w8 (an
// option changes no parameter, and the e4m3 banks have one layout) and drops u_train as well (the tile option decides its banks' shape).
void drop_banks(fcn8s_model* m, bool keep_w8 = false)
{
    if (!m->u_cache.empty() || !m->wbf16_cache.empty()) hipStreamSynchronize(m->stream);
    m->u_cache.clear(); m->wbf16_cache.clear();
    m->bank_stale.clear(); m->banks_stale = false;
    if (!keep_w8) m->w8_valid.clear();
}
// Whether a frozen model holds anything made from its parameters: a bank of any of the three kinds.  The padded / phase-packed kernels of
// prepare_forward_weights and the fingerprint frozen_fp are made in the pass that makes the first of them.  This one rule answers both
// questions forward() asks: "is there something the fingerprint guard must protect" and "must this pass rebuild and take the fingerprint".
static bool keeps_banks(const fcn8s_model* m)
{
    return !m->u_cache.empty() || !m->wbf16_cache.empty() || !m->w8_valid.empty();
}
// Everything that belongs to the arithmetic of one precision: this step's forward banks (u_train -- a mode whose forward pass does not refresh
// a bank must never find an old one), the frozen banks, the padded copies, and fp8_infer's weight banks (its calibration stays: it describes
// the parameters, not the mode).  Clearing u_train here is defensive: today every backward path that reads one of its banks also needs the
// Winograd V (or the DFT bank, fft6_ready) that the SAME pass's forward wrote, and that forward refreshed the bank first -- no sequence of calls
// reaches an old one.  It keeps that true for a path added later, and frees the banks of a mode that is no longer on.
void drop_precision_state(fcn8s_model* m)
{
    hipStreamSynchronize(m->stream);
    m->u_train.clear();
    drop_banks(m);
    drop_shape_copies(m);
    m->w8.clear();
}

int ensure_workspace(fcn8s_model* m, int N, int H, int W)
{
    int rc = check_shape(m, N, H, W); if (rc) return rc;
    if (m->arena && m->N == N && m->H == H && m->W == W) return FCN8S_OK;
    drop_arena(m);
    drop_shape_copies(m);
    WsPlan pl;
    plan_workspace(m, N, H, W, pl);
    if (!m->arena.grow(pl.bytes, m->stream, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, "workspace hipMalloc failed: out of memory");
    carve_workspace(m, N, H, W, pl);
    return FCN8S_OK;
}
// fcn8s_predict_tta: every pass runs in one arena of at least `bytes` (the largest pass's plan), re-carved when the pass shape changes.  The bf16_train
// copies are kept and only their borders zeroed again (g16_for); the training-only copies of the bf16 forward modes (xbf16) are dropped on a re-plan.
int ensure_workspace_at_least(fcn8s_model* m, int N, int H, int W, size_t bytes)
{
    int rc = check_shape(m, N, H, W); if (rc) return rc;
    const bool same = m->arena && m->N == N && m->H == H && m->W == W;
    if (same && m->arena.bytes() >= bytes) return FCN8S_OK;
    WsPlan pl;
    plan_workspace(m, N, H, W, pl);
    bytes = std::max(bytes, pl.bytes);
    if (m->arena.bytes() < bytes) {
        drop_arena(m);
        if (!m->arena.grow(bytes, m->stream, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, "workspace hipMalloc failed: out of memory");
    }
    if (!same) drop_shape_copies(m, true);
    carve_workspace(m, N, H, W, pl);
    return FCN8S_OK;
}

float* A(fcn8s_model* m, const char* n) { return m->acts.at(n).p; }

// ---- the last transposed conv (16x16, stride 8) as one GEMM over output blocks -----------------------------------------------
// (layout and algebra: PixMap in fcn8s_internal.h, tconv_*_kernel in elementwise.hip).  The s*s sub-pixel phases of tconv_fwd give every
// phase a 20-column GEMM on a 32-wide MFMA tile through the generic predicated kernel (37 TFLOP/s); as ONE GEMM with rows = output
// blocks, K = 4C and 64C columns it runs on the LDS-DMA kernels, and so do its two gradients.
const float* LG(fcn8s_model* m) { return (m->tconv_gemm && m->logits_b) ? m->logits_b : m->acts.at("logits").p; }
const PixMap* LGM(fcn8s_model* m) { return (m->tconv_gemm && m->logits_b) ? &m->pm : nullptr; }
IgemmArgs tg_rows_gemm(const float* x, int ldx, int K, const float* w, float* y, int ncols, long long rows)
{
    IgemmArgs a{};
    a.x = x; a.w = w; a.y = y;
    a.N = 1; a.Ma = (int)rows; a.Mb = 1; a.M = rows;
    a.Hi = (int)rows; a.Wi = 1; a.Cin = K; a.ldx = ldx;
    a.KW = 1; a.in_scale = 1; a.tap_step = 1; a.tap_off = 0; a.Ktot = K;
    a.Ho = (int)rows; a.Wo = 1; a.Cout = ncols; a.ldy = ncols;
    a.out_scale = 1; a.phases_x = 1; a.alpha = 1.f; a.mask_scale = 1.f;
    return a;
}
void tconv_gemm_fwd(fcn8s_model* m)
{
    hipStream_t s = m->stream;
    const int C = m->C, NC = 64 * C, KP = m->tg_kp;
    const long long rows = (long long)m->N * m->pm.QH * m->pm.QW;
    ProfScope ps(m, "tconv_fwd", 2.0 * rows * 4 * C * NC, 4.0 * rows * (4.0 * C + NC));
    launch_tconv_pack_gemm(Wp(m, "fc7_pool4_pool3_conv2d_trans/kernel"), Wp(m, "fc7_pool4_pool3_conv2d_trans/bias"), m->tg_b2, m->tg_b2t, m->tg_bias, C, 8, KP, s);
    launch_tconv_im2col(m->acts.at("a3").p, m->tg_A, m->N, m->H / 8, m->W / 8, C, KP, s);
    IgemmArgs a = tg_rows_gemm(m->tg_A, KP, 4 * C, m->tg_b2, m->logits_b, NC, rows);
    a.split = split_of(m);
    a.bias = m->tg_bias;
    launch_igemm(a, 1, s);
}
void tconv_gemm_dgrad(fcn8s_model* m)
{
    hipStream_t s = m->stream;
    const int C = m->C, NC = 64 * C, KP = m->tg_kp;
    const long long rows = (long long)m->N * m->pm.QH * m->pm.QW;
    ProfScope ps(m, "tconv_dgrad", 2.0 * rows * NC * KP, 4.0 * rows * (NC + KP));
    IgemmArgs a = tg_rows_gemm(m->dlogits_b, NC, NC, m->tg_b2t, m->tg_dA, KP, rows);
    a.split = split_of(m);
    a.batched = 1;                                   // one slab: takes the plain (16-byte store) epilogue
    launch_igemm(a, 1, s);
    launch_tconv_col2im(m->tg_dA, m->da3, m->N, m->H / 8, m->W / 8, C, KP, s);
}
void tconv_gemm_wgrad(fcn8s_model* m)
{
    hipStream_t s = m->stream;
    const int C = m->C, NC = 64 * C, KP = m->tg_kp;
    const long long rows = (long long)m->N * m->pm.QH * m->pm.QW;
    ProfScope ps(m, "tconv_wgrad", 2.0 * rows * KP * NC, 4.0 * rows * (NC + KP));
    WgradArgs g{}; g.split = split_of(m);
    g.A = m->tg_A; g.B = m->dlogits_b; g.C = m->tg_db2;
    g.N = 1; g.Pa = 1; g.Pb = (int)rows; g.P = rows;
    g.Ha = 1; g.Wa = (int)rows; g.Adim = KP; g.lda = KP; g.Areal = KP;
    g.Bdim = NC; g.ldb = NC; g.KW = 1; g.a_scale = 1; g.tap_off = 0; g.ntaps = 1; g.ldc = NC; g.alpha = 1.f; g.colsum = nullptr;
    g.c_uninitialized = 1;
    launch_wgrad(g, s);
    launch_tconv_unpack_dw(m->tg_db2, m->d_grads + m->params[m->index.at("fc7_pool4_pool3_conv2d_trans/kernel")].offset, C, 8, s);
}

// ---- forward ------------------------------------------------------------------------
int stage_inputs(fcn8s_model* m, const void* images, int dtype, const uint8_t* labels, int where,
                 const void** img_dev, const uint8_t** lab_dev)
{
    const size_t npix = (size_t)m->N * m->H * m->W;
    if (where == FCN8S_HOST) {
        const size_t ib = npix * 3 * (dtype == FCN8S_IMG_U8 ? 1 : 4);
        HIPCHK(m, hipMemcpyAsync(m->d_images, images, ib, hipMemcpyHostToDevice, m->stream));
        *img_dev = m->d_images;
        if (labels) {
            HIPCHK(m, hipMemcpyAsync(m->d_labels, labels, npix, hipMemcpyHostToDevice, m->stream));
            *lab_dev = m->d_labels;
        } else *lab_dev = nullptr;
    } else { *img_dev = images; *lab_dev = labels; }
    return FCN8S_OK;
}

void prepare_forward_weights(fcn8s_model* m)
{
    hipStream_t s = m->stream;
    prof_derived(m, "prepare_forward_weights");
    launch_pad_cin(Wp(m, "conv1_1/filter"), m->d_w1pad, 9, 3, 4, m->widths[0], s);
    launch_tconv_phase_pack(Wp(m, "fc7_conv2d_trans/kernel"), m->d_tph[0], 4, 2, m->C, s);
    launch_tconv_phase_pack(Wp(m, "fc7_pool4_conv2d_trans/kernel"), m->d_tph[1], 4, 2, m->C, s);
    launch_tconv_phase_pack(Wp(m, "fc7_pool4_pool3_conv2d_trans/kernel"), m->d_tph[2], 16, 8, m->C, s);
}

// Whether the backward pass routes d(pool_b) through the argmax bytes inside the Winograd transform of conv_b_last (then neither dZ
// nor the conv's full-resolution output is ever read again): the plan's fact, and a forward pass that kept the bytes.  `last`: the block's last conv.
bool pool_backward_fused(const Layer& last, bool pooled_by_transform) { return pooled_by_transform && last.pool_in_transform; }

// One SAME convolution with bf16-rounded operands and fp32 accumulation on the bf16 MFMA (gemm_bf16.hip), fp32 bias / ReLU / dropout epilogue,
// fp32 output: fc6 / fc7 of FCN8S_PREC_BF16_FC, and conv3_1 .. conv5_3 as well in FCN8S_PREC_BF16_FWD.  Returns false if no bf16 kernel
// takes the shape (the caller then uses the fp32 path).
struct Bf16LayerIo {
    const unsigned short* xb = nullptr;                  // the padded bf16 copy of `in`, already made (256 x 256 kernel only)
    unsigned short* yb = nullptr; int yb_pad = 0;        // bf16_train: the consumer's padded bf16 copy of the output, written by the epilogue
    long long xb_ps = 0, yb_ps = 0;                      // plane strides of xb / yb (bf16_train's per-layer copies: channel-chunk planes), 0 = [rows][C]
    bool any_shape = false;                              // bf16_train: 64- / 128-column tiles and a partial last row tile are taken too
    bool allow_small = true;                             // the 128 x 128 kernel may take what the 256 x 256 one does not
    int drop = 0; float keep_prob = 1.f; uint32_t stream_id = 0;      // dropout behind the ReLU (fc6 / fc7)
};
bool bf16_conv_layer(fcn8s_model* m, const char* tag, const Layer& L, const float* in, float* out, hipStream_t s, const Bf16LayerIo& io = Bf16LayerIo())
{
    const unsigned short* xb_ready = io.xb; unsigned short* yb = io.yb; const int yb_pad = io.yb_pad, drop = io.drop; const long long xb_ps = io.xb_ps, yb_ps = io.yb_ps;
    const bool any_shape = io.any_shape, allow_small = io.allow_small; const float keep_prob = io.keep_prob; const uint32_t stream_id = io.stream_id;
    const int N = m->N, h = L.h, w = L.w, cin = L.cin, cout = L.cout, k = L.K;
    const float *wk = m->d_params + L.w_off, *bias = m->d_params + L.b_off;
    const int K = k * k * cin;
    const long long Mrows = (long long)N * h * w;
    const bool big = conv_bf16_256_ok(Mrows, cin, cout, any_shape ? 3 : m->bf16_gemm256);      // 256-row tiles, LDS-DMA, staggered wave groups
    if (!big && (!allow_small || cin % 32 || cout % 128)) return false;
    const size_t wneed = (size_t)K * cout;
    if (!m->d_wbf16.grow(wneed * sizeof(unsigned short), s, &m->ws_allocs)) return false;
    // weights: bf16, K-tile-major blocks for the 128 x 128 kernel or transposed [Cout][K] for the 256 x 256 one; with frozen parameters
    // (evaluation / serving loops) each layer's copy is made once and kept
    unsigned short* wbuf = m->d_wbf16;
    bool have = false;
    if (m->frozen) {
        const std::string key = std::string(L.name) + (big ? "#t" : "#b");
        DeviceBuf<unsigned short>& c = m->wbf16_cache[key];
        if (c && !m->bank_stale.count("w:" + key)) { wbuf = c; have = true; }
        else if (c) { wbuf = c; m->bank_stale.erase("w:" + key); }                         // kept storage: refilled below
        else if (c.grow(wneed * sizeof(unsigned short), s, &m->ws_allocs)) wbuf = c;       // (out of memory: the shared copy, rebuilt per pass)
    }
    if (!have) { ProfScope ps(m, "weight_relayout", 0, 6.0 * K * cout);
                 prof_derived(m, big ? "w_to_bf16_t_kernel" : "w_to_bf16_tiles_kernel");
                 if (big) launch_w_to_bf16_t(wk, wbuf, K, cout, s); else launch_w_to_bf16_tiles(wk, wbuf, K, cout, s); }
    const int pad = big ? (k - 1) / 2 : 0;
    const size_t nin = (size_t)N * (h + 2 * pad) * (w + 2 * pad) * cin;
    if (nin % 8 == 0 && !(big && xb_ready)) m->d_abf16.grow(nin * sizeof(unsigned short), s, &m->ws_allocs);      // (out of memory: the paths below that need no copy)
    const double M = (double)Mrows;
    if (big && (xb_ready || (m->d_abf16 && m->d_abf16.elems() >= nin))) {
        if (!xb_ready) { ProfScope ps(m, "weight_relayout", 0, 4.0 * Mrows * cin + 2.0 * nin); launch_f32_to_bf16_padded(in, m->d_abf16, N, h, w, cin, pad, s); }
        Bf16Conv256Args g{};
        g.xp = xb_ready ? xb_ready : m->d_abf16; g.wt = wbuf; g.bias = bias; g.y = out;
        g.N = N; g.H = h; g.W = w; g.Cin = cin; g.Cout = cout; g.K = k;
        g.relu = 1; g.dropout = drop; g.keep_prob = keep_prob; g.seed = m->seed; g.stream_id = stream_id; g.any_shape = any_shape ? 1 : 0; g.mask_scale = 1.f; g.yb = yb; g.yb_pad = yb_pad;
        g.xp_ps = xb_ready ? xb_ps : 0; g.yb_ps = yb_ps;
        g.rows_bn = m->bf16_rows_bn;
        g.guarded = (any_shape && xb_ready) ? 1 : 0;          // (the per-layer training copies carry guard rows; the shared inference copy does not)
        ProfScope ps(m, tag, 2.0 * M * K * cout, (out ? 4.0 : 0.0) * M * cout + (yb ? 2.0 : 0.0) * M * cout + 2.0 * M * cin + 2.0 * K * cout, any_shape ? L.name : nullptr);
        if (launch_conv_bf16_256(g, s)) return true;
    }
    if (!out) return false;
    if (!allow_small || cin % 32 || cout % 128) return false;
    if (big) { prof_derived(m, "w_to_bf16_tiles_kernel"); launch_w_to_bf16_tiles(wk, m->d_wbf16, K, cout, s); wbuf = m->d_wbf16; }      // (could not take the 256 path after all)
    Bf16ConvArgs a{};
    a.x = in; a.wt = wbuf; a.bias = bias; a.y = out;
    if (nin % 8 == 0 && m->d_abf16) {         // activations to bf16 once: the GEMM re-reads each A tile Cout/128 times
        ProfScope ps(m, "weight_relayout", 0, 6.0 * nin); launch_f32_to_bf16(in, m->d_abf16, (long long)N * h * w * cin, s); a.xh = m->d_abf16;
    }
    a.N = N; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout; a.K = k;
    a.relu = 1; a.dropout = drop; a.keep_prob = keep_prob; a.seed = m->seed; a.stream_id = stream_id;
    ProfScope ps(m, tag, 2.0 * M * K * cout, 4.0 * M * (cin + cout) + 2.0 * K * cout);
    return launch_conv_bf16(a, s);
}

// bf16_train: a guarded, zero-bordered bf16 buffer for layer `layer` out of `bufs` (allocated and zeroed on first use or when the shape grows: the
// border and the guard rows are never written again, the interior is overwritten in every pass); returns the address of padded pixel 0 or nullptr
unsigned short* g16_for(fcn8s_model* m, fcn8s_model::G16Map& bufs, const char* layer, int N, int H, int W, int C, int K, hipStream_t s)
{
    const int pad = (K - 1) / 2, Wp_ = W + 2 * pad;
    const long long G = bf16_guard_rows(K, Wp_), R = (long long)N * (H + 2 * pad) * Wp_;
    const size_t need = (size_t)(R + 2 * G) * C;
    DeviceBuf<unsigned short>& p = bufs[layer];
    bool fresh = false;
    if (!p.grow(need * sizeof(unsigned short), s, &m->ws_allocs, true, &fresh)) return nullptr;
    if (m->g16_stale.erase(std::string(&bufs == &m->xg16 ? "x:" : "d:") + layer) && !fresh) hipMemsetAsync(p, 0, need * sizeof(unsigned short), s);     // (another shape: another border)
    return p + g16_off(G, C);           // padded pixel 0 of plane 0 (planes are g16_ps() apart)
}
// the copy of layer `layer`'s INPUT (forward pass; read again by its weight gradient)
unsigned short* xg16_for(fcn8s_model* m, const char* layer, int N, int H, int W, int C, int K, hipStream_t s) { return g16_for(m, m->xg16, layer, N, H, W, C, K, s); }
// the copy of layer `layer`'s output gradient dY [N][H][W][C]: written by the kernel that produced dY if that was a bf16 data gradient
// (dyg16_filled), else converted here, once (the layer's weight gradient asks first, its data gradient finds it)
// db: the layer's bias gradient, db[c] += sum dY[., c] -- taken by the conversion kernel on its way through dY (*db_done says whether it was)
unsigned short* dyb_for(fcn8s_model* m, const char* layer, const float* dy, int N, int H, int W, int C, int K, hipStream_t s, float* db, bool* db_done)
{
    if (db_done) *db_done = false;
    unsigned short* p = g16_for(m, m->dyg16, layer, N, H, W, C, K, s);
    if (!p) return nullptr;
    if (!m->pass.dyg16_filled.count(layer)) {
        ProfScope ps(m, "bf16_convert", 0, 4.0 * N * H * W * C + 2.0 * N * H * W * C);
        if (db && launch_f32_to_bf16_padded_colsum(dy, p, db, N, H, W, C, (K - 1) / 2, s, g16_ps(N, H, W, K))) { if (db_done) *db_done = true; }
        else launch_f32_to_bf16_padded(dy, p, N, H, W, C, (K - 1) / 2, s, g16_ps(N, H, W, K));
        m->pass.dyg16_filled.insert(layer);
    }
    return p;
}

// bf16 modes, training: the layer's Winograd input transform (run for the weight gradient anyway) can write the padded bf16 copy its direct
// bf16 convolution reads -- if that convolution takes the 256 x 256 kernel and the transform is the F(6x6,3x3) one.  Returns the layer's copy
// (allocated and its border zeroed on first use) or nullptr.
unsigned short* xb_by_transform(fcn8s_model* m, const Layer& L, int N, hipStream_t s)
{
    const int H = L.h, W = L.w, Cin = L.cin, Cout = L.cout; const char* layer = L.name;
    if (!m->bf16_copy_by_transform || Cin % 8 || !L.wv || L.tile != 6) return nullptr;
    if (!conv_bf16_256_ok((long long)N * H * W, Cin, Cout, m->bf16_gemm256)) return nullptr;
    DeviceBuf<unsigned short>& p = m->xbf16[layer];
    // (sized once: the copies are dropped whenever the workspace is planned for another shape, drop_shape_copies)
    if (!p && !p.grow((size_t)N * (H + 2) * (W + 2) * Cin * sizeof(unsigned short), s, &m->ws_allocs, true)) { m->xbf16.erase(layer); return nullptr; }
    return p;
}

// What the backward pass of a Winograd layer expects from the forward pass when the forward convolution itself did not run through
// Winograd (the bf16 modes): the transformed input V (kept for the weight gradient in the Winograd domain) and, for the adjoint data
// gradient, the forward filter bank of THIS step's weights (a bank left over from an earlier step would be silently wrong).
// in_rbits_out / in_layer: the input is the ReLU output of conv `in_layer`, whose (x > 0) record the transform writes on the way (wino_input_kernel)
// xb: also fill the interior of this padded bf16 copy of x (F(6x6,3x3) layers; the caller has checked xb_by_transform_ok)
void wino_backward_operands(fcn8s_model* m, const char* layer, const float* x, const float* wk, int N, int H, int W, int Cin, int Cout, int KS, hipStream_t s,
                            unsigned* in_rbits_out = nullptr, const char* in_layer = nullptr, unsigned short* xb = nullptr)
{
    const int tile = wino_tile_for(m, H, W, KS);
    if (!tile) return;
    auto it = m->acts.find(std::string("wv:") + layer);
    if (it == m->acts.end()) return;
    const int P = wino_alpha(tile, KS) * wino_alpha(tile, KS), nsub2 = wino_nsub(KS) * wino_nsub(KS), Kg = nsub2 * Cin;
    const long long T = wino_tiles(tile, N, H, W);
    { ProfScope ps(m, "wino_transform", 0, 4.0 * ((double)N * H * W * Cin * nsub2 + (double)P * T * Kg) + (xb ? 2.0 * N * H * W * Cin : 0.0));
      if (xb) launch_wino_input_xb(x, it->second.p, xb, N, H, W, Cin, s, in_rbits_out);
      else launch_wino_input(tile, x, it->second.p, N, H, W, Cin, KS, s, KS == 3 ? in_rbits_out : nullptr);
      if (in_rbits_out && in_layer && KS == 3) m->pass.rbits_ok.insert(in_layer); }
    const std::string key = std::string(layer) + "#" + std::to_string(tile);
    if ((KS == 3 && tile == 6) || (KS == 7 && tile == 4)) {
        DeviceBuf<float>& tu = m->u_train[key];
        if (tu.grow((size_t)P * Kg * Cout * sizeof(float), s)) { ProfScope ps(m, "wino_transform", 0, (double)(KS * KS + P * nsub2) * 4 * Cin * Cout); prof_derived(m, "wino_filter_kernel"); launch_wino_filter(tile, wk, tu, Cin, Cout, KS, s); }
        else m->u_train.erase(key);
    }
}

// ---- FCN8S_PREC_FP8_INFER ------------------------------------------------------------------------------------------------------------------------
static inline bool fp8_mode(const fcn8s_model* m) { return m && m->precision == FCN8S_PREC_FP8_INFER; }
// the modes that ride on the direct path (winograd_min_cin = 0, winograd_fc6 = 0 while they are on)
static inline bool direct_mode(int precision) { return precision == FCN8S_PREC_BF16_TRAIN || precision == FCN8S_PREC_FP8_INFER; }
const char* const kFp8Layers[FCN8S_FP8_LAYERS] = {"conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3",
                                                  "conv5_1", "conv5_2", "conv5_3", "fc6", "fc7"};
// the fp32 tensor that is layer L's input, its map's down-sampling factor and width index
const char* const kFp8Inputs[FCN8S_FP8_LAYERS] = {"conv1_1", "pool1", "conv2_1", "pool2", "conv3_1", "conv3_2", "pool3", "conv4_1", "conv4_2", "pool4",
                                                  "conv5_1", "conv5_2", "pool5", "fc6"};
const int kFp8InDiv[FCN8S_FP8_LAYERS] = {1, 2, 2, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32};
const int kFp8InWidth[FCN8S_FP8_LAYERS] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5};
static int fp8_layer(const char* name)
{
    for (int i = 0; i < FCN8S_FP8_LAYERS; ++i) if (!strcmp(name, kFp8Layers[i])) return i;
    return -1;
}
// E(a): the smallest integer e with a <= 448 2^e; E(0) = 0
static int fp8_exponent_host(float a)
{
    if (!(a > 0.f)) return 0;
    int e = ilogb((double)a) - 8;
    while ((double)a > ldexp(448.0, e)) ++e;
    while ((double)a <= ldexp(448.0, e - 1)) --e;
    return e;
}
static int fp8_ex(const fcn8s_model* m, const char* layer) { return fp8_exponent_host(m->fp8_amax[fp8_layer(layer)]); }
// parameters changed: the calibration no longer describes them
static void fp8_clear_calibration(fcn8s_model* m) { if (m) m->fp8_calibrated = false; }
// the average: while theta and the shadow have changed places (fcn8s_ema_swap) nothing trains
static int ema_refuse_swapped(fcn8s_model* m, const char* who)
{
    return fail(m, FCN8S_ERR_STATE, std::string(who) + ": the averaged weights are live (fcn8s_ema_swap); swap back before training");
}
// w = (float)(1 - d_t), d_t = warmup ? min(d, (1 + t) / (10 + t)) : d in double, t = the global step after the update
static float ema_one_minus_decay(double d, int warmup, int64_t t)
{
    if (warmup) { const double r = (1.0 + (double)t) / (10.0 + (double)t); if (r < d) d = r; }
    return (float)(1.0 - d);
}
static int fp8_refuse_training(fcn8s_model* m, const char* who)
{
    return fail(m, FCN8S_ERR_STATE, std::string(who) + ": the fp8_infer precision is inference only (evaluation, prediction); switch to another precision with "
                                    "fcn8s_set_precision to train");
}
// the e4m3 copies a pass uses: key, channels, consumer kernel size, down-sampling of the map (the 14 layer inputs and the copies the pools of blocks 1, 2, 5 read)
struct Q8Spec { std::string key; int C, K, div; };
static std::vector<Q8Spec> q8_specs(const fcn8s_model* m)
{
    std::vector<Q8Spec> v;
    for (int L = 0; L < FCN8S_FP8_LAYERS; ++L) v.push_back({kFp8Layers[L], m->widths[kFp8InWidth[L]], L == 12 ? m->fc6k : (L == 13 ? 1 : 3), kFp8InDiv[L]});
    v.push_back({"pool1in", m->widths[0], 3, 1}); v.push_back({"pool2in", m->widths[1], 3, 2}); v.push_back({"pool5in", m->widths[4], 3, 16});
    return v;
}
static size_t q8_bytes(int N, int H, int W, int C, int K) { const int pad = (K - 1) / 2; return (size_t)N * (H + 2 * pad) * (W + 2 * pad) * C; }
// copy `key` holds at least `bytes` (grown, never shrunk; a new buffer gets its border from the next q8_for)
static bool q8_grow(fcn8s_model* m, const std::string& key, size_t bytes, hipStream_t s)
{
    Q8Buf& b = m->q8[key];
    bool fresh = false;
    if (!b.p.grow(bytes, s, &m->ws_allocs, false, &fresh)) return false;
    if (fresh) b.pad = -1;
    return true;
}
// the padded e4m3 copy `key` for a K x K consumer on an H x W map of C channels, codes with exponent ex (nullptr: out of memory).  The producer writes every
// interior position in every pass; when the geometry changes (another shape, a multi-scale pass) only the border of the new geometry is zeroed -- repeated
// passes of one shape allocate and clear nothing.
static Q8Buf* q8_for(fcn8s_model* m, const std::string& key, int N, int H, int W, int C, int K, int ex, hipStream_t s)
{
    const int pad = (K - 1) / 2;
    if (!q8_grow(m, key, q8_bytes(N, H, W, C, K), s)) return nullptr;
    Q8Buf& b = m->q8[key];
    const long long R = (long long)N * (H + 2 * pad) * (W + 2 * pad);
    if (b.N != N || b.H != H || b.W != W || b.C != C || b.pad != pad) {
        launch_zero_border_fp8(b.p, C / 64, R * 64, N, H, W, pad, s);
        b.N = N; b.H = H; b.W = W; b.C = C; b.pad = pad;
    }
    b.ps = R * 64; b.ex = ex;
    return &b;
}
// a layer's quantized weight bank: rebuilt in every pass of a model that is not frozen, once while it is
static const W8Bank* w8_for(fcn8s_model* m, const char* layer, const char* wname, int KK, int Cin, int Cout, hipStream_t s)
{
    W8Bank& b = m->w8[layer];
    const size_t wbytes = (size_t)KK * Cin * Cout, need = wbytes + 8 * (size_t)Cout;
    bool fresh = false;
    if (!b.wq.grow(need, s, &m->ws_allocs, false, &fresh)) return nullptr;
    if (fresh) {
        m->w8_valid.erase(layer);
        b.ew = reinterpret_cast<int*>(b.wq + wbytes); b.amax = reinterpret_cast<unsigned*>(b.wq + wbytes + 4 * (size_t)Cout);
    }
    if (!(m->frozen && m->w8_valid.count(layer))) {
        ProfScope ps(m, "fp8_quantize_w", 0, 8.0 * wbytes + (double)wbytes, layer);
        launch_w_to_fp8(Wp(m, wname), b.wq, b.ew, b.amax, KK * Cin, Cout, s);
        if (m->frozen) m->w8_valid.insert(layer);
    }
    return &b;
}
// one FP8 convolution: the input copy of `layer` (written by its producer in this pass, or converted here from the fp32 tensor x), output as fp32 y and / or
// into the consumer's copy yq (codes with yq->ex)
static int fp8_conv(fcn8s_model* m, const char* group, const char* layer, const float* x, int N, int H, int W, int Cin, int Cout, int K,
                    float* y, const Q8Buf* yq, int yq_pad, hipStream_t s)
{
    const int Lx = fp8_layer(layer);
    const std::string ln(layer);
    const bool fc = ln == "fc6" || ln == "fc7";
    const std::string wname = ln + (fc ? "/weights" : "/filter"), bname = ln + "/biases";
    const int ex = fp8_ex(m, layer);
    Q8Buf* xq = q8_for(m, ln, N, H, W, Cin, K, ex, s);
    if (!xq) return fail(m, FCN8S_ERR_OOM, "fp8_infer: hipMalloc of " + ln + "'s e4m3 input copy failed");
    if (!m->pass.q8_filled.count(ln)) {
        // the fp32 input must have been written by this pass (conv1_1, pool3, pool4): never quantize a stale buffer
        if (Lx < 0 || m->pass.y_unwritten.count(kFp8Inputs[Lx]))
            return fail(m, FCN8S_ERR_STATE, "fp8_infer: " + ln + "'s fp32 input " + (Lx < 0 ? std::string("?") : std::string(kFp8Inputs[Lx])) + " was not written by this pass");
        ProfScope ps(m, "fp8_quantize_x", 0, 5.0 * N * H * W * Cin);
        launch_f32_to_fp8_padded(x, xq->p, N, H, W, Cin, (K - 1) / 2, xq->ps, ex, s);
        m->pass.q8_filled.insert(ln);
    }
    const W8Bank* wb = w8_for(m, layer, wname.c_str(), K * K, Cin, Cout, s);
    if (!wb) return fail(m, FCN8S_ERR_OOM, "fp8_infer: hipMalloc of " + ln + "'s e4m3 weight bank failed");
    Fp8ConvArgs a;
    a.xp = xq->p; a.xp_ps = xq->ps; a.wq = wb->wq; a.ew = wb->ew; a.bias = Wp(m, bname); a.y = y;
    if (yq) { a.yq = yq->p; a.yq_ps = yq->ps; a.yq_pad = yq_pad; a.yq_exp = yq->ex; }
    a.ex = ex; a.relu = 1; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.K = K; a.M = (long long)N * H * W;
    const double M = (double)a.M;
    ProfScope ps(m, group, 2.0 * M * K * K * Cin * Cout, M * Cin + (y ? 4.0 : 0.0) * M * Cout + (yq ? 1.0 : 0.0) * M * Cout + (double)K * K * Cin * Cout, layer);
    if (!launch_conv_fp8(a, s)) return fail(m, FCN8S_ERR_SHAPE, "fp8_infer: " + ln + " does not fit the e4m3 convolution kernel");
    return FCN8S_OK;
}

// ---- forward(): one function per stage of the encoder.  forward() walks the layer table and calls them ------------------------------------------------
// What a stage reports: a status, whether it ran the layer at all (false: the next candidate's turn), whether the block's pool came out of it.
struct FwdStep { int rc = FCN8S_OK; bool done = true, pooled = false; };
static FwdStep fwd_failed(int rc) { return FwdStep{rc}; }
static FwdStep fwd_declined() { return FwdStep{FCN8S_OK, false}; }

// FCN8S_PREC_FP8_INFER, every conv but conv1_1: the output goes to the next conv's e4m3 copy, to the copy the block's pool reads (blocks 1, 2, 5: codes with the exponent of
// the pool's consumer -- amax(pool) = amax(conv), q is monotone: the byte-max pool is exact), or to fp32 (blocks 3, 4: pool3 / pool4 feed the skip heads)
static FwdStep fwd_conv_fp8(fcn8s_model* m, Layer& L, const float* x)
{
    hipStream_t s = m->stream; const int N = m->N;
    const Layer* nx = in_block_next(m->layers, L);
    const char* nxk = nx ? nx->name : (!pool_feeds_skip(L.block) ? L.pool_in : nullptr);
    const Q8Buf* yq = nullptr;
    if (nxk) {
        const char* cons = kFp8Layers[fp8_layer(L.name) + 1];           // the next FP8 layer: the next conv, or the pool's consumer
        yq = q8_for(m, nxk, N, L.h, L.w, L.cout, 3, fp8_ex(m, cons), s);
        if (!yq) return fwd_failed(fail(m, FCN8S_ERR_OOM, "fp8_infer: hipMalloc of an e4m3 copy failed"));
    }
    const int rc = fp8_conv(m, "conv3x3_fwd_fp8", L.name, x, N, L.h, L.w, L.cin, L.cout, 3, yq ? nullptr : L.y, yq, 1, s); if (rc) return fwd_failed(rc);
    if (yq) { m->pass.q8_filled.insert(nxk); m->pass.y_unwritten.insert(L.name); }
    return FwdStep{};
}

// conv1_1's special cases (L.first()): inside conv1_2's input transform, or the 64-wide gather kernel.  Declines otherwise: conv_fwd's direct path.
static FwdStep fwd_conv1_1(fcn8s_model* m, Layer& L, const float* x, bool train, const Bf16Opts& bo)
{
    hipStream_t s = m->stream; const int N = m->N, h = L.h, w = L.w, cout = L.cout; const char* nm = L.name;
    const Layer* nx = in_block_next(m->layers, L); const float* bias = m->d_params + L.b_off;
    if (L.conv1_in_next && m->conv1_in_transform && !bf16_train_mode(m) && !fp8_mode(m)) {
        // conv1_1's only reader is conv1_2's F(6x6,3x3) input transform: that transform evaluates conv1_1 on its own patches, straight from the
        // image (winograd.hip: wino_input_conv1_kernel), writes conv1_2's V -- into the buffer conv_fwd will look for it in -- and, in training,
        // the ReLU record the backward pass masks with.  conv1_1's 134 MB per image are never written or read.
        if (!train || (nx->wv && L.rb)) {
            float* vdst = nx->wv ? nx->wv : m->d_wino_v; const long long T = wino_tiles(6, N, h, w);
            ProfScope ps(m, "wino_transform", 0, 4.0 * (4.0 * N * h * w + 64.0 * T * 64.0) + (train ? 8.0 * N * h * w : 0.0), nm);
            launch_wino_input_conv1(x, m->d_w1pad, bias, vdst, N, h, w, s, train ? L.rb : nullptr);
            if (train) m->pass.rbits_ok.insert(nm);
            m->pass.fwd_v.give(nx->name); m->pass.y_unwritten.insert(nm);
            return FwdStep{};
        }
    }
    if (cout != 64) return fwd_declined();          // write-bound gather kernel (igemm.hip: conv1_glds_kernel)
    // bf16_train: conv1_2 reads this layer as its padded bf16 copy and nobody else reads it (the mask of conv1_2's data gradient is the sign of that copy): the tile kernel writes the copy and no fp32 tensor
    unsigned short* y16 = nullptr;
    if (bf16_train_mode(m) && nx && conv1_writes_bf16_only(bo, L.shape(N), nx->shape(N))) y16 = xg16_for(m, nx->name, N, h, w, cout, 3, s);
    ProfScope ps(m, "conv1_1_fwd", 2.0 * N * h * w * 27.0 * cout, 4.0 * N * h * w * 3.0 + (y16 ? 2.0 : 4.0) * N * h * w * cout, nm);
    if (!launch_conv1_fwd(x, m->d_w1pad, bias, y16 ? nullptr : L.y, m->d_w1pad + 12 * 4 * (size_t)cout, N, h, w, cout, m->conv1_tiled, s, y16, g16_ps(N, h, w, 3))) return fwd_declined();
    if (y16) { m->pass.xg16_filled.insert(nx->name); m->pass.y_unwritten.insert(nm); m->pass.in_bf16_only.insert(nx->name); }
    return FwdStep{};
}

// FCN8S_PREC_BF16_TRAIN: every convolution but conv1_1 (3 input channels) as a direct convolution with bf16-rounded operands; the
// training pass keeps the layer's padded bf16 input copy for its weight gradient (the convolution starts from that copy)
static FwdStep fwd_conv_bf16_train(fcn8s_model* m, Layer& L, const float* x, const Bf16Opts& bo)
{
    hipStream_t s = m->stream; const int N = m->N, h = L.h, w = L.w, cin = L.cin, cout = L.cout; const char* nm = L.name;
    const Layer* nx = in_block_next(m->layers, L); const ConvShape sh = L.shape(N);
    unsigned short* xb = bo.copies ? xg16_for(m, nm, N, h, w, cin, 3, s) : nullptr;
    if (xb && !m->pass.xg16_filled.count(nm)) {
        ProfScope ps(m, "bf16_convert", 0, 4.0 * N * h * w * cin + 2.0 * N * (h + 2) * (w + 2) * cin); launch_f32_to_bf16_padded(x, xb, N, h, w, cin, 1, s, g16_ps(N, h, w, 3));
    }
    // the next convolution of the block reads this output as ITS padded bf16 input: this kernel's epilogue writes that copy
    unsigned short* yb = nullptr; const char* nxk = "";
    if (out_bf16_copy(bo, nx != nullptr)) { nxk = nx->name; yb = xg16_for(m, nxk, N, h, w, cout, 3, s); }
    // the block's LAST convolution is read by its pool only: the pool then takes this output as a bf16 copy of the kernel's own geometry ("pool<b>in"),
    // picks its maxima among the bf16 values (what bf16(max of the fp32 values) is anyway) and no fp32 tensor is written
    const bool pool16 = L.last_of_block() && pool_in_bf16(bo, sh, m->layers[L.next].shape(N), L.block);
    if (pool16) { nxk = L.pool_in; yb = xg16_for(m, nxk, N, h, w, cout, 3, s); }
    // ... and if the copy is the output's only reader, the fp32 tensor is not written at all.  (yb without pool16: the in-block consumer's copy.)
    const bool only16 = yb && (pool16 || out_bf16_only(bo, sh, nx->shape(N)));
    // (launch_wgrad_bf16's limit, applied HERE, before anything is launched)
    if (!bf16_plane_fits(g16_ps(N, h, w, 3)))
        return fwd_failed(fail(m, FCN8S_ERR_SHAPE, std::string("bf16_train: a 32-channel plane of the padded bf16 copy of ") + nm + "'s input would reach 4 GiB at this batch size; use a smaller batch per GPU"));
    Bf16LayerIo io; io.allow_small = false; io.any_shape = true;
    io.xb = xb; io.xb_ps = g16_ps(N, h, w, 3); io.yb = yb; io.yb_pad = 1; io.yb_ps = g16_ps(N, h, w, 3);
    // (unreachable by rule -- every width is a multiple of 64: bf16_kernels_take -- kept as the guard for an allocation failure and a refused launch)
    if (!bf16_conv_layer(m, "conv3x3_fwd_bf16", L, x, only16 ? nullptr : L.y, s, io)) return fwd_failed(fail(m, FCN8S_ERR_SHAPE, std::string("bf16_train: ") + nm + " does not fit the bf16 convolution kernel"));
    if (yb) m->pass.xg16_filled.insert(nxk);
    if (only16) { m->pass.y_unwritten.insert(nm); if (!pool16) m->pass.in_bf16_only.insert(nxk); }
    return FwdStep{};
}

// FCN8S_PREC_BF16_FWD: conv3_1 .. conv5_3 as direct convolutions with bf16-rounded operands on the 256 x 256 bf16 kernel (the output is materialised, the block's pool
// runs as its own kernel, ReLU masks come from the activations); the backward pass stays in the Winograd domain, so the transformed input and this step's filter bank
// are made here.  Declines if no bf16 kernel takes the shape.
static FwdStep fwd_conv_bf16_fwd(fcn8s_model* m, Layer& L, const float* x, bool train)
{
    hipStream_t s = m->stream; const int N = m->N;
    // training: the transform that keeps this layer's V for the weight gradient runs first and writes the padded bf16 copy of the
    // input on the way (the convolution then starts from it; without a kept V, or in inference, the convolution converts its input itself)
    unsigned short* xb = train ? xb_by_transform(m, L, N, s) : nullptr;
    auto operands = [&]() {
        // the previous conv of the block came from the bf16 kernel too (no ReLU record): this transform of its output writes one
        const Layer* pv = in_block_prev(m->layers, L);
        unsigned* irb = (pv && pv->rb && !m->pass.rbits_ok.count(pv->name)) ? pv->rb : nullptr;
        wino_backward_operands(m, L.name, x, m->d_params + L.w_off, N, L.h, L.w, L.cin, L.cout, 3, s, irb, irb ? pv->name : nullptr, xb);
    };
    if (xb) operands();
    Bf16LayerIo io; io.allow_small = false; io.xb = xb;
    if (!bf16_conv_layer(m, "conv3x3_fwd_bf16", L, x, L.y, s, io)) return fwd_declined();
    if (train && !xb) operands();
    return FwdStep{};
}

// Every other conv: conv_fwd picks Winograd or the direct path (conv_route.h); this builds the epilogue the layer table asks for
static FwdStep fwd_conv(fcn8s_model* m, Layer& L, const float* x, bool train)
{
    const Layer* nx = in_block_next(m->layers, L);
    FwdEpi e; e.bias = m->d_params + L.b_off; e.relu = 1;
    if (train && L.rb_writer == RbWriter::self) e.relu_bits_out = L.rb;                              // its output is the next conv's input
    if (train && L.pos == 2 && m->layers[L.prev].rb_writer == RbWriter::consumer) {                  // input = conv1_1, made by the gather kernel
        e.in_relu_bits_out = m->layers[L.prev].rb; e.in_layer = m->layers[L.prev].name;
    }
    if (L.last_of_block()) {
        e.pool_out = L.pool;
        if (train) e.pool_idx = L.pidx;
        // The block's last conv output feeds only the pool.  If the output transform writes the pool (and, for training, the backward
        // pass routes through the argmax bytes), the full-resolution tensor is never read again and is not written at all
        // (2.15 GB for conv1_2 at 16 x 1024x512); fcn8s_get_activation of such a layer then returns stale data.
        e.skip_y = !train || L.pool_in_transform;
        e.gemm_out_fused64 = L.gemm_out_fused64 && m->gemm_out_fused64;
    }
    if (L.out_in_next && m->fuse_out_in && !(bf16_fwd_mode(m) && L.block >= 3) && !bf16_train_mode(m) && !fp8_mode(m) && (!train || e.relu_bits_out)) {
        // this conv and the next one both run through F(6x6,3x3) on the same tile grid: its output transform writes the next conv's
        // transformed input directly (training: into the buffer kept for that conv's weight gradient) and its own output never exists.
        // The buffer the next conv will read its V from is the one kept for its weight gradient if the workspace has one (whether or
        // not this pass trains), else the shared scratch.  (out_in_fused: the next conv keeps V -- a direct weight gradient would read
        // the activation that no longer exists.)
        e.next_v = nx->wv ? nx->wv : m->d_wino_v; e.next_layer = nx->name;
    }
    FwdStep st;
    const float* wt = L.first() ? m->d_w1pad : m->d_params + L.w_off;
    st.pooled = conv_fwd(m, L.first() ? "conv1_1_fwd" : "conv3x3_fwd", x, wt, L.y, m->N, L.h, L.w, L.cin, L.cout, 3, e, m->stream, L.real_cin, L.name);
    return st;
}

// A block's pool behind its last conv L (cons: the pool's consumer, the next block's first conv or fc6) unless that conv's output transform wrote it
// (pooled): fp8_infer's byte max, bf16_train's routed pool on the bf16 copies, or the plain kernel with or without routing bytes
static FwdStep fwd_pool(fcn8s_model* m, const Layer& L, const Layer& cons, const float* x, bool train, bool fp8, bool pooled, const Bf16Opts& bo)
{
    hipStream_t s = m->stream; const int N = m->N, b = L.block - 1, h = L.h, w = L.w, cin = L.cout; const char* pn = L.pool_name;
    if (fp8) {
        m->pass.pool_fused[b] = false; m->pass.pool_routed[b] = false;
        if (!pool_feeds_skip(L.block)) {
            // byte max of the last conv's e4m3 copy straight into the consumer's copy (conv<b+2>_1, pad 1; fc6, pad (k - 1) / 2)
            const int ck = cons.K;
            Q8Buf* yq = q8_for(m, cons.name, N, h / 2, w / 2, cin, ck, fp8_ex(m, cons.name), s);
            if (!yq) return fwd_failed(fail(m, FCN8S_ERR_OOM, "fp8_infer: hipMalloc of an e4m3 copy failed"));
            const Q8Buf& xi = m->q8[L.pool_in];
            { ProfScope ps(m, "maxpool_fwd_fp8", 0, 1.25 * N * h * w * cin); launch_maxpool_fp8(xi.p, xi.ps, yq->p, yq->ps, N, h, w, cin, (ck - 1) / 2, s); }
            m->pass.q8_filled.insert(cons.name); m->pass.y_unwritten.insert(pn);
        } else { ProfScope ps(m, "maxpool_fwd", 0, 4.0 * N * h * w * cin * 1.25); launch_maxpool_fwd(x, L.pool, N, h, w, cin, s); }
        return FwdStep{};
    }
    m->pass.pool_fused[b] = pooled && train;
    m->pass.pool_routed[b] = false;
    const ConvShape last = L.shape(N), csh = cons.shape(N);
    if (!pooled && bf16_train_mode(m) && pool_routes(bo, last)) {
        // bf16_train, training: the pool keeps its routing bytes (the backward pass reads one byte per window instead of the block's last activation)
        // and writes the consumer's padded bf16 copy itself -- conv<b+2>_1 (pad 1) or fc6 (pad 3); pool1, pool2 and pool5 have no other reader, so
        // with option bf16_acts their fp32 tensors are not written (pool3 / pool4 feed the fp32 skip heads)
        const int ck = cons.K;
        unsigned short* yb = pool_out_bf16(bo, last, csh) ? xg16_for(m, cons.name, N, h / 2, w / 2, cin, ck, s) : nullptr;
        const bool only16 = yb && pool_out_bf16_only(bo, last, csh, L.block);
        auto pi = m->xg16.find(L.pool_in);
        const bool in16 = only16 && pool_reads_bf16(bo, last, csh, L.block) && pi != m->xg16.end() && pi->second && m->pass.xg16_filled.count(L.pool_in);      // the last conv wrote only its bf16 copy
        ProfScope ps(m, "maxpool_fwd", 0, (in16 ? 2.0 : 4.0) * N * h * w * cin + 4.0 * N * h * w * cin * (only16 ? 0.0625 : 0.3125) + (yb ? 0.5 * N * h * w * cin : 0.0));
        if (in16) launch_maxpool_fwd_route16(pi->second + g16_off(bf16_guard_rows(3, w + 2), cin), g16_ps(N, h, w, 3), L.pidx, N, h, w, cin, s, yb, (ck - 1) / 2, g16_ps(N, h / 2, w / 2, ck));
        else launch_maxpool_fwd_route(x, only16 ? nullptr : L.pool, L.pidx, N, h, w, cin, s, yb, (ck - 1) / 2, g16_ps(N, h / 2, w / 2, ck),
                                      /*round16=*/pool_feeds_skip(L.block) ? 0 : 1);
        m->pass.pool_routed[b] = true; pooled = true;
        if (yb) m->pass.xg16_filled.insert(cons.name);
        if (only16) { m->pass.y_unwritten.insert(pn); m->pass.in_bf16_only.insert(cons.name); }
    }
    if (!pooled) {
        // a block whose last conv did not run through the Winograd output transform (bf16 modes) but whose backward pass does run in the
        // Winograd domain: keep the same routing bytes, so that d(pool) is routed inside wino_dout_kernel and dZ is never written
        const bool route = train && cin % 4 == 0 && L.pool_in_transform;
        ProfScope ps(m, "maxpool_fwd", 0, 4.0 * N * h * w * cin * (route ? 1.3125 : 1.25));
        if (route) { launch_maxpool_fwd_route(x, L.pool, L.pidx, N, h, w, cin, s); m->pass.pool_fused[b] = true; }
        else launch_maxpool_fwd(x, L.pool, N, h, w, cin, s);
    }
    return FwdStep{};
}

// Monte-Carlo dropout inference (fcn8s_predict_mc): forward() runs the encoder and the two skip heads once, then fc6 -> fc7 -> decoder once per sample with
// dropout on at keep_prob in a prediction pass (train = false), sample s on counter streams base + 2 s (fc6) and base + 2 s + 1 (fc7), and hands each
// sample's logits to after_sample
struct McLoop { int samples = 1; uint32_t stream_base = 0; std::function<void(int)> after_sample; };

// fc6 and fc7 on pool5 (x), each precision's own way.  mc_stream: a sample of fcn8s_predict_mc -- dropout without a training pass, on this counter stream
static FwdStep fwd_fc(fcn8s_model* m, const float* x, float keep_prob, bool train, bool fp8, const Bf16Opts& bo, const uint32_t* mc_stream = nullptr)
{
    hipStream_t s = m->stream; const int N = m->N;
    const Layer &F6 = m->layers[13], &F7 = m->layers[14];
    const int h5 = F6.h, w5 = F6.w;
    float *w6 = m->d_params + F6.w_off, *b6 = m->d_params + F6.b_off, *w7 = m->d_params + F7.w_off, *b7 = m->d_params + F7.b_off;
    const bool drop = (train || mc_stream) && keep_prob < 1.f;
    m->drop_stream = mc_stream ? *mc_stream : (uint32_t)(2 * m->step);
    Bf16LayerIo io6, io7;          // (the bf16 precisions)
    io6.drop = io7.drop = drop; io6.keep_prob = io7.keep_prob = keep_prob; io6.stream_id = m->drop_stream; io7.stream_id = m->drop_stream + 1;
    if (fp8) {
        // fc6 writes fc7's e4m3 copy only; fc7 writes fp32 for the fc7_1x1 head
        const Q8Buf* q7 = q8_for(m, F7.name, N, h5, w5, F7.cin, 1, fp8_ex(m, F7.name), s);
        if (!q7) return fwd_failed(fail(m, FCN8S_ERR_OOM, "fp8_infer: hipMalloc of an e4m3 copy failed"));
        int rc = fp8_conv(m, "fc6_fwd_fp8", F6.name, x, N, h5, w5, F6.cin, F6.cout, F6.K, nullptr, q7, 0, s); if (rc) return fwd_failed(rc);
        m->pass.q8_filled.insert(F7.name); m->pass.y_unwritten.insert(F6.name);
        rc = fp8_conv(m, "fc7_fwd_fp8", F7.name, F6.y, N, h5, w5, F7.cin, F7.cout, 1, F7.y, nullptr, 0, s); if (rc) return fwd_failed(rc);
    } else if (bf16_train_mode(m)) {
        unsigned short* xb6 = bo.copies ? xg16_for(m, F6.name, N, h5, w5, F6.cin, F6.K, s) : nullptr;
        if (xb6 && !m->pass.xg16_filled.count(F6.name)) { ProfScope ps(m, "bf16_convert", 0, 6.0 * N * h5 * w5 * F6.cin); launch_f32_to_bf16_padded(x, xb6, N, h5, w5, F6.cin, (F6.K - 1) / 2, s, g16_ps(N, h5, w5, F6.K)); }
        unsigned short* xb7 = bo.copies ? xg16_for(m, F7.name, N, h5, w5, F7.cin, 1, s) : nullptr;
        const bool fuse7 = xb7 != nullptr && fc7_in_from_fc6(bo);      // fc7's input copy comes out of fc6's epilogue (16-byte stores since the tile kernel's epilogue goes through LDS)
        io6.allow_small = io7.allow_small = false; io6.any_shape = io7.any_shape = true;
        io6.xb = xb6; io6.xb_ps = g16_ps(N, h5, w5, F6.K); io6.yb = fuse7 ? xb7 : nullptr; io6.yb_pad = 0; io6.yb_ps = g16_ps(N, h5, w5, 1);
        io7.xb = xb7; io7.xb_ps = g16_ps(N, h5, w5, 1);
        // (both unreachable by rule, as the conv layers' text: kept as the guards for an allocation failure and a refused launch)
        if (!bf16_conv_layer(m, "fc6_fwd_bf16", F6, x, F6.y, s, io6)) return fwd_failed(fail(m, FCN8S_ERR_SHAPE, "bf16_train: fc6 does not fit the bf16 convolution kernel"));
        if (xb7 && !fuse7) { ProfScope ps(m, "bf16_convert", 0, 6.0 * N * h5 * w5 * F7.cin); launch_f32_to_bf16_padded(F6.y, xb7, N, h5, w5, F7.cin, 0, s, g16_ps(N, h5, w5, 1)); }
        if (!bf16_conv_layer(m, "fc7_fwd_bf16", F7, F6.y, F7.y, s, io7)) return fwd_failed(fail(m, FCN8S_ERR_SHAPE, "bf16_train: fc7 does not fit the bf16 convolution kernel"));
    } else if (m->precision == FCN8S_PREC_BF16_FC || bf16_fwd_mode(m)) {
        // config 5: bf16-rounded operands, fp32 accumulate, fp32 epilogue and output (gemm_bf16.hip)
        bf16_conv_layer(m, "fc6_fwd_bf16", F6, x, F6.y, s, io6);
        // the fp32 gradients of fc6 run in the Winograd domain and want the transformed input and this step's filter bank
        if (train) wino_backward_operands(m, F6.name, x, w6, N, h5, w5, F6.cin, F6.cout, F6.K, s);
        bf16_conv_layer(m, "fc7_fwd_bf16", F7, F6.y, F7.y, s, io7);
    } else {
        { FwdEpi e; e.bias = b6; e.relu = 1; e.dropout = drop; e.keep = keep_prob; e.stream_id = m->drop_stream;
          conv_fwd(m, "fc6_fwd", x, w6, F6.y, N, h5, w5, F6.cin, F6.cout, F6.K, e, s, 0, F6.name); }
        { FwdEpi e; e.bias = b7; e.relu = 1; e.dropout = drop; e.keep = keep_prob; e.stream_id = m->drop_stream + 1;
          conv_fwd(m, "fc7_fwd", F6.y, w7, F7.y, N, h5, w5, F7.cin, F7.cout, 1, e, s); }
    }
    return FwdStep{};
}

// What one forward() call is asked for: a training pass or a prediction pass, its dropout, x0 already written (tta_input ran: the preprocess kernel is
// skipped), fcn8s_fp8_calibrate's fp32 pass of the fp8_infer mode, fcn8s_predict_mc's sample loop
struct FwdCall { float keep_prob = 1.f; bool train = false, x0_written = false, calibrating = false; const McLoop* mc = nullptr; };

int forward(fcn8s_model* m, const void* img_dev, int dtype, const FwdCall& call)
{
    const float keep_prob = call.keep_prob; const bool train = call.train; const McLoop* mc = call.mc;
    t_deterministic = m->deterministic;
    hipStream_t s = m->stream;
    const int N = m->N, H = m->H, W = m->W, C = m->C;
    // FCN8S_PREC_FP8_INFER: evaluation / prediction through the e4m3 kernels; the calibration pass (fcn8s_fp8_calibrate) is the fp32 direct path
    const bool fp8 = fp8_mode(m) && !train && !call.calibrating;
    if (fp8 && !m->fp8_calibrated)
        return fail(m, FCN8S_ERR_STATE, "fp8_infer: the model has no FP8 calibration (never calibrated, or its parameters changed since): run fcn8s_fp8_calibrate "
                                        "(Engine.calibrate_fp8 / FCN8s.calibrate_fp8) or restore one with fcn8s_fp8_set_calibration first");
    m->pass.begin_forward(fp8);
    bool guard_pending = false;
    if (m->frozen && keeps_banks(m) && !m->banks_stale) {
        // the caller promised constant parameters; a cheap strided fingerprint catches the promise being broken through a side
        // door (a torch optimizer or copy_ over views of ext_params): the kept banks -- Winograd filters, bf16 kernels, e4m3 weights --
        // are then rebuilt instead of reused.
        // The check does not hold the pass up: the fingerprint is taken first on the stream, the pass is enqueued behind it with the kept
        // banks, and the host compares when the (long finished) copy is looked at -- at the end of this function; a mismatch repeats the pass.
        launch_fingerprint(m->d_params, (long long)m->total, m->d_fp, s);
        m->h_fp.grow(sizeof(unsigned long long), s);          // (no pinned memory: the synchronous comparison below)
        if (m->h_fp && !m->fp_event) hipEventCreateWithFlags(&m->fp_event, hipEventDisableTiming);
        if (m->h_fp && m->fp_event) {
            hipMemcpyAsync(m->h_fp, m->d_fp, sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
            hipEventRecord(m->fp_event, s);
            guard_pending = true;
        } else {
            unsigned long long fp = 0;
            hipMemcpyAsync(&fp, m->d_fp, sizeof fp, hipMemcpyDeviceToHost, s);
            hipStreamSynchronize(s);
            if (fp != m->frozen_fp) drop_banks(m);
        }
    }
    const bool fill_fp = m->frozen && (!keeps_banks(m) || m->banks_stale);          // (banks_stale: kept storage, contents to be rebuilt)
    if (!m->frozen || fill_fp) prepare_forward_weights(m);        // frozen and the kept banks still valid: so are the padded / phase-packed kernels
    m->fwd_train = train;
    // bf16_train, evaluation / prediction (round 6): the pass takes the TRAINING pass's data flow -- every layer's input as a padded bf16 copy written by its
    // producer's epilogue (no fp32 conv -> conv tensor, no conversion pass), the flat-position kernel, pools on the bf16 copies -- instead of fp32 tensors converted
    // layer by layer for the tile kernel: 13.3 -> 9.3 ms per 16 x 1024x512 batch, 1.55 -> 1.18 ms per single image (profiles/r06_bf16_infer.txt).  Same products in the same order as the training pass:
    // its logits are the training pass's bit for bit (keep_prob 1).  What it keeps for a backward pass that never comes (routing bytes) costs one byte per window.
    const Bf16Opts bo = bf16_opts(m, train);          // (read by the bf16_train branches alone.  bo.copies: a training pass, or option bf16_infer_copies)
    if (!call.x0_written) { ProfScope ps(m, "preprocess", 0, (double)N * H * W * (16 + (dtype ? 12 : 3))); launch_preprocess(img_dev, dtype, A(m, "x0"), (long long)N * H * W, s); }
    const float* x = A(m, "x0");
    size_t k = 0;
    for (int b = 0; b < 5; ++b) {
        FwdStep st;
        for (; m->layers[k].block == b + 1; ++k) {          // each conv: the first stage that takes it
            Layer& L = m->layers[k];
            if (fp8 && !L.first()) st = fwd_conv_fp8(m, L, x);
            else {
                st = L.first() ? fwd_conv1_1(m, L, x, train, bo) : fwd_declined();
                if (!st.done && bf16_train_mode(m) && !L.first()) st = fwd_conv_bf16_train(m, L, x, bo);
                if (!st.done && bf16_fwd_mode(m) && b >= 2) st = fwd_conv_bf16_fwd(m, L, x, train);
                if (!st.done) st = fwd_conv(m, L, x, train);
            }
            if (st.rc) return st.rc;
            x = L.y;
        }
        const Layer& last = m->layers[k - 1];         // the block's last conv; m->layers[k]: the pool's consumer (the next block's first conv, or fc6)
        st = fwd_pool(m, last, m->layers[k], x, train, fp8, st.pooled, bo);
        if (st.rc) return st.rc;
        x = last.pool;
    }
    const int h5 = H / 32, w5 = W / 32;
    // decoder (fcn8s_tensorflow.py:171-233): the two skip heads, which read the encoder alone, and the part behind fc7
    auto skip_heads = [&]() {
        { FwdEpi e; e.bias = Wp(m, "pool3_1x1/bias"); e.alpha = 0.0001f;
          conv_fwd(m, "score1x1_fwd", A(m, "pool3"), Wp(m, "pool3_1x1/kernel"), A(m, "p3"), N, H / 8, W / 8, m->widths[2], C, 1, e, s); }
        { FwdEpi e; e.bias = Wp(m, "pool4_1x1/bias"); e.alpha = 0.01f;
          conv_fwd(m, "score1x1_fwd", A(m, "pool4"), Wp(m, "pool4_1x1/kernel"), A(m, "p4"), N, H / 16, W / 16, m->widths[3], C, 1, e, s); }
    };
    auto fc7_head_and_upsampling = [&]() {
        { FwdEpi e; e.bias = Wp(m, "fc7_1x1/bias");
          conv_fwd(m, "score1x1_fwd", A(m, "fc7"), Wp(m, "fc7_1x1/kernel"), A(m, "s7"), N, h5, w5, m->widths[6], C, 1, e, s); }
        tconv_fwd(m, A(m, "s7"), m->d_tph[0], Wp(m, "fc7_conv2d_trans/bias"), A(m, "p4"), A(m, "a4"), N, h5, w5, C, 4, 2, s);
        tconv_fwd(m, A(m, "a4"), m->d_tph[1], Wp(m, "fc7_pool4_conv2d_trans/bias"), A(m, "p3"), A(m, "a3"), N, H / 16, W / 16, C, 4, 2, s);
        if (m->tconv_gemm && m->logits_b) tconv_gemm_fwd(m);
        else tconv_fwd(m, A(m, "a3"), m->d_tph[2], Wp(m, "fc7_pool4_pool3_conv2d_trans/bias"), nullptr, A(m, "logits"), N, H / 8, W / 8, C, 16, 8, s);
        m->logits_nhwc_valid = !(m->tconv_gemm && m->logits_b);
    };
    if (!mc) {
        { const FwdStep st = fwd_fc(m, x, keep_prob, train, fp8, bo); if (st.rc) return st.rc; }
        skip_heads();
        fc7_head_and_upsampling();
    } else {
        // What the repeated part reads and nothing in it writes: pool5 (or fc6's padded bf16 copy of it, a buffer of its own), p3 and p4 -- arena items of their own;
        // the transform-domain scratch (wino_v / wino_m) is filled again from pool5 by every sample's fc6 and is no input of it.
        skip_heads();
        for (int k = 0; k < mc->samples; ++k) {
            const uint32_t sid = mc->stream_base + 2u * (uint32_t)k;
            const FwdStep st = fwd_fc(m, x, keep_prob, train, fp8, bo, &sid); if (st.rc) return st.rc;
            fc7_head_and_upsampling();
            mc->after_sample(k);
        }
    }
    if (fill_fp) {                        // this pass (re)built the cache: remember what it was built from
        launch_fingerprint(m->d_params, (long long)m->total, m->d_fp, s);
        hipMemcpyAsync(&m->frozen_fp, m->d_fp, sizeof m->frozen_fp, hipMemcpyDeviceToHost, s);
        hipStreamSynchronize(s);
        m->banks_stale = false;
    }
    if (guard_pending) {
        hipEventSynchronize(m->fp_event);
        if (*m->h_fp != m->frozen_fp) {            // the parameters changed behind the library's back: this pass used stale banks -- again, without them
            drop_banks(m);
            return forward(m, img_dev, dtype, call);
        }
    }
    m->have_forward = true; m->train_mode = train; m->keep_prob = keep_prob; m->mc_masks = mc != nullptr;
    return FCN8S_OK;
}

// forward() as an entry point runs it: with the thread's deferred-error slot empty in front (a call that returned early on this thread may have left it
// set), and what a launcher deferred during the pass as the result
int run_forward(fcn8s_model* m, const void* img_dev, int dtype, const FwdCall& call)
{
    take_deferred_error(nullptr);
    const int rc = forward(m, img_dev, dtype, call);
    if (rc) { take_deferred_error(nullptr); return rc; }
    return deferred_rc(m);
}
// One whole pass over a batch of the caller's: the workspace for its shape, the inputs on the device (*lab_dev: where the labels are), forward()
int run_pass(fcn8s_model* m, const void* images, int dtype, const uint8_t* labels, int N, int H, int W, int where, const FwdCall& call,
             const uint8_t** lab_dev = nullptr)
{
    int rc = ensure_workspace(m, N, H, W); if (rc) return rc;
    const void* img; const uint8_t* lab;
    rc = stage_inputs(m, images, dtype, labels, where, &img, &lab); if (rc) return rc;
    if (lab_dev) *lab_dev = lab;
    return run_forward(m, img, dtype, call);
}

// ---- what fcn8s_predict_tta, fcn8s_predict_mc and fcn8s_predict_crf share ----------------------------------------------------------------
// A call of several passes runs with frozen parameters: each transformed filter bank is built once and every pass after the first reuses it.  A model
// that was not frozen keeps the banks' storage after the call with its contents marked stale (bank_stale, banks_stale; fp8_infer: its weight banks
// are re-quantized): the next call rebuilds each bank once into it, allocating nothing.  Whichever way the call returns.
struct FrozenForCall {
    fcn8s_model* const m; const bool was_frozen;
    explicit FrozenForCall(fcn8s_model* model) : m(model), was_frozen(model->frozen) { m->frozen = true; }
    ~FrozenForCall()
    {
        if (was_frozen) return;
        for (auto& kv : m->u_cache) m->bank_stale.insert("u:" + kv.first);
        for (auto& kv : m->wbf16_cache) m->bank_stale.insert("w:" + kv.first);
        m->banks_stale = true;
        m->w8_valid.clear();
        m->frozen = false;
    }
};

// A call's scratch in one of the model's grown-only buffers: take() every item in its order (each starts 256-byte aligned), grow() once, then ptr()
// resolves an item (nullptr for one of 0 bytes).  A call that takes nothing allocates nothing.
struct Scratch {
    DeviceBuf<char>& buf; size_t total = 0;
    struct Item { size_t off = 0, bytes = 0; };
    Item take(size_t bytes) { const Item it{total, bytes}; total += align_up(bytes, 256); return it; }
    bool grow(fcn8s_model* m) { return !total || buf.grow(total, m->stream, &m->ws_allocs); }
    template <class T> T* ptr(const Item& it) const { return it.bytes ? (T*)(buf.get() + it.off) : nullptr; }
};

// The host / device boundary of a prediction call.  FCN8S_HOST: the images and every output that was asked for are items of the scratch, staged in
// by stage() and copied out by copy_out(); FCN8S_DEVICE: the caller's own pointers, and neither takes a byte.  input() / output() in the scratch's order.
struct PredictIo {
    fcn8s_model* m; Scratch& sc; const bool host;
    struct Port { void* user = nullptr; size_t bytes = 0; Scratch::Item item; } in, outs[3];
    int nouts = 0;
    PredictIo(fcn8s_model* model, Scratch& scratch, int where) : m(model), sc(scratch), host(where == FCN8S_HOST) {}
    void input(const void* images, size_t bytes) { in = Port{const_cast<void*>(images), bytes, sc.take(host ? bytes : 0)}; }
    int output(void* user, size_t bytes) { outs[nouts] = Port{user, bytes, sc.take(host && user ? bytes : 0)}; return nouts++; }
    // (behind sc.grow())
    const void* images_dev() const { return host ? sc.ptr<void>(in.item) : in.user; }
    int stage() { if (host) HIPCHK(m, hipMemcpyAsync(sc.ptr<void>(in.item), in.user, in.bytes, hipMemcpyHostToDevice, m->stream)); return FCN8S_OK; }
    void* dev(int o) const { return host ? sc.ptr<void>(outs[o].item) : outs[o].user; }          // (nullptr: this output was not asked for)
    void split(int o, bool argmax, float** sm, long long** am) const { *sm = argmax ? nullptr : (float*)dev(o); *am = argmax ? (long long*)dev(o) : nullptr; }
    int copy_out()
    {
        for (int o = 0; host && o < nouts; ++o)
            if (outs[o].user) HIPCHK(m, hipMemcpyAsync(outs[o].user, dev(o), outs[o].bytes, hipMemcpyDeviceToHost, m->stream));
        if (host) HIPCHK(m, hipStreamSynchronize(m->stream));
        return FCN8S_OK;
    }
};

// The refusals they share, under the caller's name; each caller keeps its own rules between them, in its own order
int check_predict_args(fcn8s_model* m, const char* who, int dtype, int where)
{
    if (dtype != FCN8S_IMG_U8 && dtype != FCN8S_IMG_F32) return fail(m, FCN8S_ERR_BAD_ARG, std::string(who) + ": unknown image dtype");
    if (where != FCN8S_HOST && where != FCN8S_DEVICE) return fail(m, FCN8S_ERR_BAD_ARG, std::string(who) + ": `where` must be FCN8S_HOST or FCN8S_DEVICE");
    return FCN8S_OK;
}
int check_predict_shape(fcn8s_model* m, const char* who, int N, int H, int W)
{ return N <= 0 || H <= 0 || W <= 0 ? fail(m, FCN8S_ERR_SHAPE, std::string(who) + ": N, H and W must be positive") : FCN8S_OK; }
int check_padded_shape(fcn8s_model* m, const char* who, const char* which, int N, int Hp, int Wp)
{ return (double)N * Hp * Wp > (double)(1LL << 31) ? fail(m, FCN8S_ERR_SHAPE, std::string(who) + ": " + which + " padded shape is too large to plan") : FCN8S_OK; }
// how the last pass's logits (LG) are laid out: the blocked layout of the GEMM route, or plain NHWC over the padded map
PixMap logits_map(fcn8s_model* m, int Hp, int Wp) { return LGM(m) ? *LGM(m) : PixMap{0, Hp, Wp, 0, 0, 0}; }

const char* kDecoderKernels[6] ={"pool3_1x1/kernel", "pool4_1x1/kernel", "fc7_1x1/kernel", "fc7_conv2d_trans/kernel",
                                  "fc7_pool4_conv2d_trans/kernel", "fc7_pool4_pool3_conv2d_trans/kernel"};

// the scratch of a configured training loss (fcn8s_set_loss, fcn8s_set_boundary_loss) in its effective mode: state + histograms, and for OHEM
// the l_p buffer of npix floats
int ensure_loss_ws(fcn8s_model* m, long long npix, int mode)
{
    const size_t need = LOSS_SCRATCH_BYTES + (mode == 2 ? (size_t)npix * sizeof(float) : 0);
    return m->loss_ws.grow(need, m->stream, &m->ws_allocs) ? FCN8S_OK : fail(m, FCN8S_ERR_OOM, "the training loss's scratch cannot be allocated");
}

// the Lovász sort's scratch (fcn8s_set_lovasz), grown only
int ensure_lovasz_ws(fcn8s_model* m, const LovaszLayout& y)
{
    return m->lov_ws.grow(y.bytes, m->stream, &m->ws_allocs) ? FCN8S_OK : fail(m, FCN8S_ERR_OOM, "the Lovasz sort's scratch cannot be allocated");
}

int compute_loss(fcn8s_model* m, const uint8_t* lab_dev, float l2_rate, bool with_grad)
{
    hipStream_t s = m->stream;
    const long long npix = (long long)m->N * m->H * m->W;
    const int nb = softmax_xent_blocks(npix);
    // the last pass's logits and their gradient in the layout they live in (blocked: the GEMM route of the last transposed conv), for every launch below
    const bool blk = m->tconv_gemm && m->logits_b;
    const float* lg = blk ? m->logits_b : A(m, "logits");
    float* dlg = blk ? m->dlogits_b : m->dlogits;
    const PixMap* pm = blk ? &m->pm : nullptr;
    const bool bnd = with_grad && m->bnd_R > 0;               // evaluation keeps the reference's loss
    const int mode = with_grad ? (m->loss_mode ? m->loss_mode : bnd ? 1 : 0) : 0;    // the boundary weighting alone: the weighted mode, d_cw holds ones
    const bool focal = with_grad && m->focal_gamma > 0.f;      // the focal launch in the cross-entropy's place (mode is 0 or 1: OHEM is refused with it)
    if (focal && mode == 2) return fail(m, FCN8S_ERR_STATE, "fcn8s_set_focal: the focal loss does not combine with OHEM");
    if (mode || focal) { int rc = ensure_loss_ws(m, npix, mode ? mode : 1); if (rc) return rc; }       // (focal: the state that holds |V| for fcn8s_get_loss_stats)
    if (focal && !m->focal_ws.grow(focal_xent_scratch_bytes(), s, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, "the focal loss's scratch cannot be allocated");
    if (bnd) {
        // the distance codes of THIS loss's labels (those the device-side augmentation left), in front of the loss on the same stream
        if ((long long)m->H * m->W >= (1LL << 31)) return fail(m, FCN8S_ERR_SHAPE, "fcn8s_set_boundary_loss: an image has to have fewer than 2^31 pixels");
        if (!m->d_btab || !m->d_cw) return fail(m, FCN8S_ERR_STATE, "fcn8s_set_boundary_loss: the table is missing");
        if (!m->d_bcodes.grow((size_t)npix, s, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, "the boundary weighting's distance codes cannot be allocated");
        ProfScope ps(m, "boundary_distance", 0, 2.0 * (double)npix);      // the labels in, the codes out
        launch_boundary_distance(lab_dev, m->N, m->H, m->W, m->bnd_R, m->d_bcodes, s);
    }
    OhemState* st = mode ? (OhemState*)m->loss_ws.get() : nullptr;
    const bool lov = with_grad && m->lov_on;                    // evaluation keeps the reference's loss here too
    const bool lov_sort = lov && m->lov_w != 0.f;
    const float gscale = lov ? m->lov_ce * (1.0f / (float)npix) : 1.0f / (float)npix;    // (exactly 1 / npix at lov_ce == 1)
    LovaszLayout ly;
    if (lov_sort) {
        if (npix / (m->lov_per_image ? m->N : 1) >= (1LL << 31)) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_lovasz: a segment holds 2^31 pixels or more");
        ly = lovasz_layout(npix, m->lov_per_image ? m->N : 1, m->C);
        int rc = ensure_lovasz_ws(m, ly); if (rc) return rc;
    }
    // bytes: the logits once (+ dlogits) and the labels; OHEM reads the logits and labels twice and writes + reads l_p (its refinement
    // passes, 4 bytes per pixel each when min_kept decides the threshold, are not counted)
    const double xbytes = (mode == 2 ? (double)npix * (m->C * 4 * 3 + 2 + 8) : (double)npix * (m->C * 4 * (with_grad ? 2 : 1) + 1)) + (bnd ? (double)npix : 0.0);   // (+ the codes)
    if (focal) {
        // L_foc and its gradient: one launch plus a one-block reduction that leave what the cross-entropy's launch leaves -- the loss sum as the one
        // partial finalize_loss reads, d_lastbias (set, all 64 columns defined by the memset), |V| in the loss state -- so that everything behind is untouched
        ProfScope ps(m, "focal_xent", 0, focal_xent_bytes(npix, m->C, bnd));
        hipMemsetAsync(m->d_lastbias, 0, 64 * sizeof(float), s);
        launch_focal_xent(lg, dlg, lab_dev, mode ? (const float*)m->d_cw : nullptr,
                          bnd ? (const uint8_t*)m->d_bcodes : nullptr, bnd ? (const float*)m->d_btab : nullptr, pm, m->N, npix, m->C,
                          m->focal_gamma, gscale, m->focal_ws, m->d_partials, nullptr, (OhemState*)m->loss_ws.get(), m->d_lastbias, s);
    } else
    { ProfScope ps(m, "softmax_xent", 0, xbytes);
      if (with_grad) hipMemsetAsync(m->d_lastbias, 0, 64 * sizeof(float), s);
      if (mode) {
          XentEx x; x.cw = m->d_cw; x.st = st; x.hist = (unsigned*)(m->loss_ws + sizeof(OhemState));
          x.lbuf = mode == 2 ? (float*)(m->loss_ws + LOSS_SCRATCH_BYTES) : nullptr;
          if (lov) x.ce_scale = m->lov_ce;
          if (bnd) { x.codes = m->d_bcodes; x.ptab = m->d_btab; }
          launch_softmax_xent_ex(lg, lab_dev, dlg, m->d_partials, npix, m->C, gscale, s,
                                 m->d_lastbias, pm, m->N, x, mode == 2 ? m->ohem_thresh : 0.f, (long long)m->ohem_min_kept);
      } else
          launch_softmax_xent(lg, lab_dev, with_grad ? dlg : nullptr, m->d_partials, npix, m->C,
                              gscale, s, with_grad ? m->d_lastbias : nullptr, pm, m->N); }
    if (with_grad) { m->last_loss_mode = focal ? 1 : mode; m->bnd_last = bnd ? npix : 0; }     // (focal: |V| is reported as in the weighted mode)
    const float* reg = nullptr;
    if (l2_rate != 0.f) {
        hipMemsetAsync(m->d_regsum, 0, sizeof(float), s);
        for (auto k : kDecoderKernels) launch_sumsq(Wp(m, k), m->d_regsum, (long long)P(m, k).numel, s);
        reg = m->d_regsum;
    }
    launch_finalize_loss(m->d_partials, focal ? 1 : nb, npix, reg, l2_rate, m->d_loss, s, mode == 2 ? &st->kept : nullptr, with_grad ? m->d_terms : nullptr);
    if (with_grad) m->have_terms = true;
    if (lov_sort) {
        // L_lov and its gradient: keys, sort, Jaccard scan (the loss, now final), then dlogits += lov_w d L_lov / d logits and the bias column sums
        ProfScope ps(m, "lovasz", 0, lovasz_bytes(npix, m->C, m->lov_nmask));
        launch_lovasz_loss(lg, 1, lab_dev, pm, m->N, npix, ly, m->lov_all, m->d_lovmask, m->lov_ws, nullptr, m->d_terms,
                           m->lov_ce, m->lov_w, m->d_loss, s);
        launch_lovasz_backward(lg, 1, lab_dev, pm, m->N, npix, ly, m->lov_ws, m->lov_w, 1, dlg,
                               m->d_lastbias, s);
    } else if (lov)
        launch_lovasz_total(m->d_terms, m->lov_ce, m->d_loss, s);
    if (with_grad) m->have_kd = false;
    if (with_grad && m->kd_w != 0.f) {
        // L_kd and its gradient against the bound target rows (fcn8s_forward_loss has checked the binding): dlogits += kd_w d L_kd / d logits, then
        // the loss, the term and the bias column sums -- all in front of the loss copy below
        if (!m->kd_ws.grow(soft_targets_scratch_bytes(), s, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, "the soft-target term's scratch cannot be allocated");
        ProfScope ps(m, "soft_targets", 0, soft_targets_bytes(npix, m->C, m->kd_K));
        launch_soft_targets(lg, dlg, m->kd_probs, lab_dev, pm, m->N, npix,
                            m->C, m->kd_K, m->kd_stride, m->kd_w, m->kd_T, m->kd_all, m->kd_ws, m->d_loss, m->d_terms + 3, m->d_lastbias, s);
        m->have_kd = true;
    }
    if (with_grad) m->have_ent = false;
    if (with_grad && m->ent_w != 0.f) {
        // L_ent and its gradient on the student's own prediction: dlogits += ent_w d L_ent / d logits, then the loss, the term and the bias column
        // sums -- all in front of the loss copy below
        if (!m->ent_ws.grow(entropy_term_scratch_bytes(), s, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, "the entropy term's scratch cannot be allocated");
        ProfScope ps(m, "entropy_term", 0, entropy_term_bytes(npix, m->C));
        launch_entropy_term(lg, dlg, lab_dev, pm, m->N, npix, m->C, m->ent_K,
                            m->ent_set, m->ent_first, m->ent_w, m->ent_ws, m->d_loss, m->d_terms + 4, m->d_lastbias, 1, s);
        m->have_ent = true;
    }
    // The loss is final here, a third of the way into a training step: queue its copy now, so that fcn8s_read_loss waits for this
    // point of the stream only and the host can go on queueing the next step while the backward pass runs (the reference fetches
    // the loss every step, fcn8s_tensorflow.py:554-578; waiting for the whole stream left the GPU idle for ~2 ms per step).
    m->loss_copied = m->h_loss && m->loss_ev && hipMemcpyAsync(m->h_loss, m->d_loss, sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess &&
                     hipEventRecord(m->loss_ev, s) == hipSuccess;
    m->l2_rate = l2_rate; m->have_loss = true;
    return FCN8S_OK;
}

// ---- backward --------------------------------------------------------------------------
void prepare_backward_weights(fcn8s_model* m)
{
    hipStream_t s = m->stream;
    ProfScope ps(m, "weight_relayout", 0, 8.0 * ((double)m->widths[5] * m->widths[6] +
                                                 (double)m->C * (m->widths[2] + m->widths[3] + m->widths[6])));
    // (the 3x3 layers' and fc6's flipped + transposed kernels are made on demand in conv_dgrad: the adjoint Winograd data gradients read
    // the forward filter banks)
    launch_flip_transpose(Wp(m, "fc7/weights"), WTp(m, "fc7/weights"), 1, m->widths[5], m->widths[6], s);
    launch_flip_transpose(Wp(m, "pool3_1x1/kernel"), WTp(m, "pool3_1x1/kernel"), 1, m->widths[2], m->C, s);
    launch_flip_transpose(Wp(m, "pool4_1x1/kernel"), WTp(m, "pool4_1x1/kernel"), 1, m->widths[3], m->C, s);
    launch_flip_transpose(Wp(m, "fc7_1x1/kernel"), WTp(m, "fc7_1x1/kernel"), 1, m->widths[6], m->C, s);
}

void l2_grad(fcn8s_model* m, const char* kernel)
{
    if (m->l2_rate != 0.f) launch_axpy(Gp(m, kernel), Wp(m, kernel), m->l2_rate, (long long)P(m, kernel).numel, m->stream);
}

// the gradients of bucket b are final behind the last kernel queued on `s`: record the event fcn8s_bucket_wait hands to other streams
void mark_bucket_final(fcn8s_model* m, int b, hipStream_t s)
{
    if (!m->bucket_ev[b]) hipEventCreateWithFlags(&m->bucket_ev[b], hipEventDisableTiming);
    hipEventRecord(m->bucket_ev[b], s);
    m->bucket_final[b] = true;
}

// backward phase 0: the decoder and fc7's weight gradient (bucket 0 = {fc7, decoder})
void backward_head(fcn8s_model* m)
{
    hipStream_t s = m->stream;
    const int N = m->N, H = m->H, W = m->W, C = m->C;
    const int h5 = H / 32, w5 = W / 32, h4 = H / 16, w4 = W / 16, h3 = H / 8, w3 = W / 8;
    const float inv_keep = (m->train_mode && m->keep_prob < 1.f) ? 1.f / m->keep_prob : 1.f;
    hipMemsetAsync(m->d_grads, 0, m->total * sizeof(float), s);
    prepare_backward_weights(m);
    // logits = tconv16x16s8(a3)
    const bool blk = m->tconv_gemm && m->logits_b;
    if (blk) tconv_gemm_wgrad(m); else tconv_wgrad(m, A(m, "a3"), m->dlogits, Gp(m, "fc7_pool4_pool3_conv2d_trans/kernel"), N, h3, w3, C, 16, 8, s);
    launch_axpy(Gp(m, "fc7_pool4_pool3_conv2d_trans/bias"), m->d_lastbias, 1.f, C, s);      // column sums of dlogits, from the loss kernel
    if (blk) tconv_gemm_dgrad(m); else tconv_dgrad(m, m->dlogits, Wp(m, "fc7_pool4_pool3_conv2d_trans/kernel"), m->da3, N, h3, w3, C, 16, 8, s);
    l2_grad(m, "fc7_pool4_pool3_conv2d_trans/kernel");
    // a3 = tconv4x4s2(a4) + p3 ; p3 = conv1x1(pool3 * 1e-4)
    conv_wgrad(m, "score1x1_wgrad", A(m, "pool3"), m->da3, Gp(m, "pool3_1x1/kernel"), Gp(m, "pool3_1x1/bias"), N, h3, w3, m->widths[2], C, 1, 0.0001f, s);
    l2_grad(m, "pool3_1x1/kernel");
    { DgradEpi e; e.alpha = 0.0001f; conv_dgrad(m, "score1x1_dgrad", m->da3, WTp(m, "pool3_1x1/kernel"), m->gskip3, N, h3, w3, C, m->widths[2], 1, e, s); }
    tconv_wgrad(m, A(m, "a4"), m->da3, Gp(m, "fc7_pool4_conv2d_trans/kernel"), N, h4, w4, C, 4, 2, s);
    launch_colsum(m->da3, Gp(m, "fc7_pool4_conv2d_trans/bias"), (long long)N * h3 * w3, C, s);
    tconv_dgrad(m, m->da3, Wp(m, "fc7_pool4_conv2d_trans/kernel"), m->da4, N, h4, w4, C, 4, 2, s);
    l2_grad(m, "fc7_pool4_conv2d_trans/kernel");
    // a4 = tconv4x4s2(s7) + p4 ; p4 = conv1x1(pool4 * 1e-2)
    conv_wgrad(m, "score1x1_wgrad", A(m, "pool4"), m->da4, Gp(m, "pool4_1x1/kernel"), Gp(m, "pool4_1x1/bias"), N, h4, w4, m->widths[3], C, 1, 0.01f, s);
    l2_grad(m, "pool4_1x1/kernel");
    { DgradEpi e; e.alpha = 0.01f; conv_dgrad(m, "score1x1_dgrad", m->da4, WTp(m, "pool4_1x1/kernel"), m->gskip4, N, h4, w4, C, m->widths[3], 1, e, s); }
    tconv_wgrad(m, A(m, "s7"), m->da4, Gp(m, "fc7_conv2d_trans/kernel"), N, h5, w5, C, 4, 2, s);
    launch_colsum(m->da4, Gp(m, "fc7_conv2d_trans/bias"), (long long)N * h4 * w4, C, s);
    tconv_dgrad(m, m->da4, Wp(m, "fc7_conv2d_trans/kernel"), m->ds7, N, h5, w5, C, 4, 2, s);
    l2_grad(m, "fc7_conv2d_trans/kernel");
    // s7 = conv1x1(fc7)
    conv_wgrad(m, "score1x1_wgrad", A(m, "fc7"), m->ds7, Gp(m, "fc7_1x1/kernel"), Gp(m, "fc7_1x1/bias"), N, h5, w5, m->widths[6], C, 1, 1.f, s);
    l2_grad(m, "fc7_1x1/kernel");
    { DgradEpi e; e.mask = A(m, "fc7"); e.mask_scale = inv_keep;
      conv_dgrad(m, "score1x1_dgrad", m->ds7, WTp(m, "fc7_1x1/kernel"), m->gbuf[0], N, h5, w5, C, m->widths[6], 1, e, s); }
    // fc7
    conv_wgrad(m, "fc7_wgrad", A(m, "fc6"), m->gbuf[0], Gp(m, "fc7/weights"), Gp(m, "fc7/biases"), N, h5, w5, m->widths[5], m->widths[6], 1, 1.f, s, 0, "fc7");
    mark_bucket_final(m, 0, s);
}

// backward phase 1: fc7's data gradient, fc6 (bucket 1 = {fc6}: final behind its weight gradient, before its data gradient is queued)
void backward_fc6(fcn8s_model* m)
{
    hipStream_t s = m->stream;
    const int N = m->N, H = m->H, W = m->W;
    const int h5 = H / 32, w5 = W / 32;
    const float inv_keep = (m->train_mode && m->keep_prob < 1.f) ? 1.f / m->keep_prob : 1.f;
    { DgradEpi e; e.mask = A(m, "fc6"); e.mask_scale = inv_keep; e.w_fwd = Wp(m, "fc7/weights"); e.yb_layer = "fc6"; e.yb_K = m->fc6k;      // (w_fwd + the layer name: the bf16_train branch of conv_dgrad)
      conv_dgrad(m, "fc7_dgrad", m->gbuf[0], WTp(m, "fc7/weights"), m->gbuf[1], N, h5, w5, m->widths[6], m->widths[5], 1, e, s, "fc7"); }
    // fc6
    conv_wgrad(m, "fc6_wgrad", A(m, "pool5"), m->gbuf[1], Gp(m, "fc6/weights"), Gp(m, "fc6/biases"), N, h5, w5, m->widths[4], m->widths[5], m->fc6k, 1.f, s, 0, "fc6");
    mark_bucket_final(m, 1, s);
    { DgradEpi e; e.w_fwd = Wp(m, "fc6/weights"); e.lazy_wt = 1;      // (flipped + transposed copy only if the adjoint path is not taken)
      conv_dgrad(m, "fc6_dgrad", m->gbuf[1], WTp(m, "fc6/weights"), m->gbuf[0], N, h5, w5, m->widths[5], m->widths[4], m->fc6k, e, s, "fc6"); }
    m->gcur = 0;   // gbuf[0] holds d(pool5)
}

// blocks [b_hi .. b_lo] (1-based VGG block numbers), going backwards
void backward_blocks(fcn8s_model* m, int b_hi, int b_lo)
{
    hipStream_t s = m->stream;
    const int N = m->N;
    for (int k = (int)m->layers.size() - 1; k >= 0; --k) {
        Layer& L = m->layers[k];
        if (L.block > b_hi || L.block < b_lo) continue;
        const int b = L.block, h = L.h, w = L.w, cw = L.cout, cin = L.cin;
        const char* nm = L.name;
        float *gw = m->d_grads + L.w_off, *gb = m->d_grads + L.b_off;
        // d(pool_b) in gbuf[gcur] -> dZ of the last conv (ReLU mask fused).  If the forward pass kept the argmax bytes and both
        // gradients of that conv run through Winograd, the routing happens inside their shared transform and dZ is never written.
        const unsigned char* pix = nullptr;
        if (L.last_of_block()) {
            if (pool_backward_fused(L, m->pass.pool_fused[b - 1])) pix = L.pidx;
            bool pool_done = false;
            if (!pix && bf16_train_mode(m) && m->train_mode && pool_bwd_writes_bf16(bf16_opts(m, true), L.shape(N))) {
                // bf16_train: nobody reads the fp32 dZ of the block's last conv -- its weight and data gradients take the padded bf16 copy, its bias gradient the
                // column sums: the pool's backward kernel writes exactly those (gbuf[gcur ^ 1] stays unwritten; the "dz" handed on below is never dereferenced)
                unsigned short* dzb = g16_for(m, m->dyg16, nm, N, h, w, cw, 3, s);
                if (dzb) {
                    ProfScope ps(m, "maxpool_bwd", 0, 4.0 * N * h * w * cw * (m->pass.pool_routed[b - 1] ? 0.3125 : 1.25) + 2.0 * N * h * w * cw);
                    pool_done = launch_maxpool_bwd_bf16(L.y, m->gbuf[m->gcur], dzb, gb, N, h, w, cw, s,
                                                        m->pass.pool_routed[b - 1] ? L.pidx : nullptr, g16_ps(N, h, w, 3));
                }
                if (pool_done) { m->pass.dyg16_filled.insert(nm); m->pass.db_taken.insert(nm); m->pass.dz_unwritten.insert(nm); m->gcur ^= 1; }
            }
            if (!pix && !pool_done) {
                ProfScope ps(m, "maxpool_bwd", 0, 4.0 * N * h * w * cw * 2.25);
                launch_maxpool_bwd(L.y, m->gbuf[m->gcur], m->gbuf[m->gcur ^ 1], N, h, w, cw, 1, s);
                m->gcur ^= 1;
            }
        }
        const float* dz = m->gbuf[m->gcur];
        const Layer* pv = in_block_prev(m->layers, L);                // the layer whose output this one reads: the conv in front of it, the pool of the block before, or the image
        const float* xin = pv ? pv->y : (L.first() ? A(m, "x0") : m->layers[L.prev].pool);
        // (whether the data gradient that follows shares this transform, and in which form, is the layer's own rule: conv_wgrad asks it)
        conv_wgrad(m, L.first() ? "conv1_1_wgrad" : "conv3x3_wgrad", xin, dz, gw, gb, N, h, w, cin, cw, 3, 1.f, s, L.real_cin, nm, pix);
        if (L.first()) break;
        DgradEpi e; e.w_fwd = m->d_params + L.w_off; e.lazy_wt = 1;
        if (pv) {                                                      // ReLU of the previous conv
            e.mask = xin; e.mask_scale = 1.f; e.yb_layer = pv->name; e.yb_K = 3;
            if (m->pass.rbits_ok.count(pv->name)) e.relu_bits_in = pv->rb;
            e.yb_only = bf16_train_mode(m) && dy_bf16_only(bf16_opts(m, true), pv->shape(N), pv->first(), L.shape(N));
            // The previous conv takes this gradient only through dM = A dZ A^T (weight gradient in the Winograd domain, adjoint data
            // gradient): the gather kernel can write dM directly.
            if (pv->dm_from_next && m->fuse_dgrad_dout && e.relu_bits_in && m->train_mode) { e.dm_out = m->d_wino_m; e.dm_out_layer = pv->name; }
        }
        else if (b == 5) e.addend = m->gskip4;                        // d(pool4) also receives the pool4_1x1 path
        else if (b == 4) e.addend = m->gskip3;                        // d(pool3) also receives the pool3_1x1 path
        conv_dgrad(m, "conv3x3_dgrad", dz, m->d_wt + L.w_off, m->gbuf[m->gcur ^ 1], N, h, w, cw, cin, 3, e, s, nm);
        m->gcur ^= 1;
    }
}

// bucket b is final when call b returns: buckets 0 and 1 (fc7 + decoder, fc6) are marked behind their weight gradients, the conv
// buckets at the end of their calls -- so that each all-reduce can start at once
int do_backward_bucket(fcn8s_model* m, int bucket)
{
    t_deterministic = m->deterministic;
    if (!m->have_loss || !m->train_mode) return fail(m, FCN8S_ERR_STATE, "fcn8s_backward_bucket: call fcn8s_forward_loss first");
    if (bucket != m->next_bucket) return fail(m, FCN8S_ERR_STATE, "fcn8s_backward_bucket: buckets must be run in order 0, 1, ... fcn8s_num_buckets() - 1");
    if (bucket == 0) {
        m->pass.begin_backward();
        for (int b = 0; b < kNumBuckets; ++b) m->bucket_final[b] = false;
        // (a caller that skipped fcn8s_apply_update after fcn8s_allreduce_bucket: the gradient buffer is about to be cleared and rewritten,
        //  so this stream first waits for whatever the library's communicator still has in flight on it)
        for (int b = 0; b < kNumBuckets; ++b)
            if (m->comm_pending[b]) { hipStreamWaitEvent(m->stream, m->comm_done[b], 0); m->comm_pending[b] = false; }
        backward_head(m);
    }
    else if (bucket == 1) backward_fc6(m);
    else if (bucket == 2) backward_blocks(m, 5, 4);
    else backward_blocks(m, 3, 1);
    if (!m->bucket_final[bucket]) mark_bucket_final(m, bucket, m->stream);
    m->next_bucket = bucket + 1;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(m, FCN8S_ERR_HIP, std::string("backward launch: ") + hipGetErrorString(e));
    return FCN8S_OK;
}

int ensure_opt_state(fcn8s_model* m)
{
    if (m->d_m) return FCN8S_OK;
    if (!m->d_m.grow(m->total * sizeof(float), m->stream) || !m->d_v.grow(m->total * sizeof(float), m->stream)) {
        m->d_m.reset(); return fail(m, FCN8S_ERR_OOM, "the optimizer's slots cannot be allocated");
    }
    HIPCHK(m, hipMemsetAsync(m->d_m, 0, m->total * sizeof(float), m->stream));
    HIPCHK(m, hipMemsetAsync(m->d_v, 0, m->total * sizeof(float), m->stream));
    return FCN8S_OK;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

size_t fcn8s_param_floats(const fcn8s_config* cfg)
{
    if (!cfg || cfg->num_classes <= 0) return 0;
    int C, widths[7], k; resolve_cfg(cfg, C, widths, k);
    std::vector<ParamInfo> t; size_t total, bo[FCN8S_MAX_BUCKETS], bn[FCN8S_MAX_BUCKETS];
    build_param_table(C, widths, k, t, total, bo, bn);
    return total;
}

int fcn8s_layout_num_params(const fcn8s_config* cfg)
{
    if (!cfg || cfg->num_classes <= 0) return 0;
    int C, widths[7], k; resolve_cfg(cfg, C, widths, k);
    std::vector<ParamInfo> t; size_t total, bo[FCN8S_MAX_BUCKETS], bn[FCN8S_MAX_BUCKETS];
    build_param_table(C, widths, k, t, total, bo, bn);
    return (int)t.size();
}
int fcn8s_layout_param(const fcn8s_config* cfg, int index, char name_out[64], int32_t* ndim, int64_t shape[4], int64_t* off)
{
    if (!cfg || cfg->num_classes <= 0) return FCN8S_ERR_BAD_ARG;
    int C, widths[7], k; resolve_cfg(cfg, C, widths, k);
    std::vector<ParamInfo> t; size_t total, bo[FCN8S_MAX_BUCKETS], bn[FCN8S_MAX_BUCKETS];
    build_param_table(C, widths, k, t, total, bo, bn);
    if (index < 0 || index >= (int)t.size()) return FCN8S_ERR_BAD_ARG;
    if (name_out) { strncpy(name_out, t[index].name.c_str(), 63); name_out[63] = 0; }
    if (ndim) *ndim = t[index].ndim;
    if (shape) for (int i = 0; i < 4; ++i) shape[i] = t[index].shape[i];
    if (off) *off = (int64_t)t[index].offset;
    return FCN8S_OK;
}
int fcn8s_layout_num_buckets(const fcn8s_config* cfg) { return (cfg && cfg->num_classes > 0) ? kNumBuckets : 0; }
int fcn8s_layout_bucket(const fcn8s_config* cfg, int bucket, size_t* off, size_t* n)
{
    if (!cfg || cfg->num_classes <= 0 || bucket < 0 || bucket >= kNumBuckets) return FCN8S_ERR_BAD_ARG;
    int C, widths[7], k; resolve_cfg(cfg, C, widths, k);
    std::vector<ParamInfo> t; size_t total, bo[FCN8S_MAX_BUCKETS], bn[FCN8S_MAX_BUCKETS];
    build_param_table(C, widths, k, t, total, bo, bn);
    if (off) *off = bo[bucket];
    if (n) *n = bn[bucket];
    return FCN8S_OK;
}

int fcn8s_create(const fcn8s_config* cfg, fcn8s_model** out)
{
    if (!cfg || !out) return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_create: null argument");
    if (cfg->num_classes <= 0 || cfg->num_classes % 4 != 0 || cfg->num_classes > 64)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_create: num_classes must be a positive multiple of 4, at most 64 (the Python facade pads other class counts)");
    fcn8s_model* m = new fcn8s_model();
    resolve_cfg(cfg, m->C, m->widths, m->fc6k);
    for (int i = 0; i < 7; ++i)
        if (m->widths[i] % 4) { delete m; return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_create: channel widths must be multiples of 4"); }
    if (m->fc6k % 2 == 0) { delete m; return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_create: fc6_ksize must be odd"); }
    m->device = cfg->device_id; m->seed = cfg->seed;
    hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) { delete m; return fail(nullptr, FCN8S_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e) + " (libfcn8s_hip needs an AMD GPU; there is no CPU fallback)"); }
    {   // the kernels are written for gfx950: up to 160 KB of LDS per workgroup (conv_bf16_256_kernel), 96 KB static in wino_out_in_kernel.  Say so
        // here, once, instead of failing every launch with a generic error on a part that has 64 KB.
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, m->device) == hipSuccess && prop.sharedMemPerBlock < FCN8S_LDS_BYTES_NEEDED) {
            const std::string msg = std::string("fcn8s_create: device ") + std::to_string(m->device) + " (" + prop.gcnArchName + ") offers " + std::to_string(prop.sharedMemPerBlock) +
                                    " bytes of LDS per workgroup; this library is written for gfx950 (MI355X) and needs " + std::to_string(FCN8S_LDS_BYTES_NEEDED);
            delete m; return fail(nullptr, FCN8S_ERR_HIP, msg);
        }
    }
    build_param_table(m->C, m->widths, m->fc6k, m->params, m->total, m->bucket_off, m->bucket_n);
    for (size_t i = 0; i < m->params.size(); ++i) m->index[m->params[i].name] = (int)i;
    // (hipMalloc'ed memory is not zero: what is read before it is first written is cleared here)
    bool ok = true;
    auto dev = [&](auto& buf, size_t n, bool zero = false) { ok = ok && buf.grow(n * sizeof(*buf.get()), nullptr, nullptr, zero); };
    if (cfg->ext_params) m->d_params = (float*)cfg->ext_params; else { dev(m->own_params, m->total, true); m->d_params = m->own_params; }
    if (cfg->ext_grads) m->d_grads = (float*)cfg->ext_grads; else { dev(m->own_grads, m->total, true); m->d_grads = m->own_grads; }
    dev(m->d_wt, m->total);
    // 12 taps x 4 channels: rows 36..47 (three padding taps of the LDS-DMA conv1_1 kernel) and the 64 floats behind them stay zero
    dev(m->d_w1pad, 12 * 4 * (size_t)m->widths[0] + 64, true);
    const size_t cc = (size_t)m->C * m->C;
    dev(m->d_tph[0], 16 * cc); dev(m->d_tph[1], 16 * cc); dev(m->d_tph[2], 256 * cc);
    {
        int cmax = 0; for (int i = 0; i < 5; ++i) cmax = std::max(cmax, m->widths[i]);
        m->ufl = 64 * (size_t)cmax * cmax;                            // F(6x6,3x3): 64 positions
        if (m->fc6k == 7) m->ufl = std::max(m->ufl, fc6_bank_floats(m->widths[4], m->widths[5]));
        dev(m->d_wino_u, m->ufl);
    }
    dev(m->d_loss, 2 + 64 + 5, true);
    m->d_regsum = m->d_loss + 1; m->d_lastbias = m->d_loss + 2; m->d_terms = m->d_loss + 2 + 64;
    dev(m->d_conf, cc, true); dev(m->d_fp, 1);
    m->tg_kp = (4 * m->C + 63) / 64 * 64;
    {
        const size_t NC = 64 * (size_t)m->C, KP = (size_t)m->tg_kp;
        dev(m->tg_b2, 4 * (size_t)m->C * NC); dev(m->tg_b2t, NC * KP); dev(m->tg_db2, KP * NC); dev(m->tg_bias, NC);
    }
    if (!ok) { fcn8s_destroy(m); return fail(nullptr, FCN8S_ERR_OOM, "fcn8s_create: out of device memory"); }
    hipStreamSynchronize(nullptr);          // the clears above: done before a caller's stream touches the buffers
    m->h_loss.grow(64, nullptr);            // (no pinned memory: the loss is read synchronously)
    if (hipEventCreateWithFlags(&m->loss_ev, hipEventDisableTiming) != hipSuccess) { m->loss_ev = nullptr; (void)hipGetLastError(); }
    *out = m;
    return FCN8S_OK;
}

int fcn8s_destroy(fcn8s_model* m)
{
    if (!m) return FCN8S_OK;
    // the communicator first: its stream is drained by polling (a dead peer ends in an abort after comm_timeout_ms), and only then is the device
    // synchronised -- the other way round a collective that waits for a peer that is gone would hold hipDeviceSynchronize until the watchdog fires
    const int rc_comm = fcn8s_comm_destroy(m);
    const std::string comm_text = rc_comm ? m->err : std::string();
    hipDeviceSynchronize();
    // the per-stream scratch of the streams this model ran on (the caller's stream may live on: what it holds is given back, the next user grows its own)
    // (the scratch is keyed by the calling device: release under the model's, whichever one the caller has current)
    m->streams_seen.insert(m->stream);
    int cur = m->device; (void)hipGetDevice(&cur);
    if (cur != m->device && hipSetDevice(m->device) != hipSuccess) (void)hipGetLastError();
    for (hipStream_t s : m->streams_seen) scratch_release(s);
    if (cur != m->device) (void)hipSetDevice(cur);
    delete m;
    // the model is gone either way; a communicator that had failed is reported once, with its reason in fcn8s_last_error(NULL)
    if (rc_comm) { g_last_error = comm_text; return rc_comm; }
    return FCN8S_OK;
}

const char* fcn8s_last_error(const fcn8s_model* m) { return m ? m->err.c_str() : g_last_error.c_str(); }

int fcn8s_freeze_params(fcn8s_model* m, int frozen)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!frozen || !m->frozen) drop_banks(m);          // entering or leaving: start from an empty cache
    m->frozen = frozen != 0;
    return FCN8S_OK;
}

int fcn8s_set_precision(fcn8s_model* m, int precision)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (precision < FCN8S_PREC_F32 || precision > FCN8S_PREC_FP8_INFER)
        return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_precision: unknown precision");
    if (precision == FCN8S_PREC_BF16_TRAIN) {
        for (int i = 0; i < 7; ++i)
            if (m->widths[i] % 64) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_precision: the bf16_train mode needs every channel width to be a multiple of 64");
    }
    if (precision == FCN8S_PREC_FP8_INFER) {
        for (int i = 0; i < 7; ++i)
            if (m->widths[i] % 64) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_precision: the fp8_infer mode needs every channel width to be a multiple of 64");
        if (m->fc6k % 2 == 0) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_precision: the fp8_infer mode needs an odd fc6 kernel size");
    }
    if (precision == FCN8S_PREC_BF16_FC || precision == FCN8S_PREC_BF16_FWD || precision == FCN8S_PREC_BF16_FWD_X2) {
        if (m->widths[4] % 32 || m->widths[5] % 128 || m->widths[6] % 128)
            return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_precision: the bf16 modes need conv5 width % 32 == 0 and fc6 / fc7 widths % 128 == 0");
    }
    if (precision != m->precision) {
        HIPCHK(m, hipStreamSynchronize(m->stream));
        drop_precision_state(m);
        // bf16_train runs every convolution but conv1_1 as a DIRECT convolution on the bf16 MFMA, forward and backward: it rides on the library's
        // direct path (no Winograd transforms, the pools as kernels of their own, ReLU masks from the activations), i.e. on the settings
        // winograd_min_cin = 0 / winograd_fc6 = 0, which it takes over while it is on (and which need another workspace)
        // (fp8_infer's calibration pass and its fp32 layers ride on the same direct path)
        const bool was = direct_mode(m->precision), now = direct_mode(precision);
        if (was != now) {
            if (now) { m->saved_wino_min_cin = m->wino_min_cin; m->saved_wino_fc6 = m->wino_fc6; m->wino_min_cin = 0; m->wino_fc6 = 0; }
            else { if (m->saved_wino_min_cin >= 0) m->wino_min_cin = m->saved_wino_min_cin; if (m->saved_wino_fc6 >= 0) m->wino_fc6 = m->saved_wino_fc6; }
            drop_arena(m);
        }
    }
    m->precision = precision;
    return FCN8S_OK;
}
int fcn8s_get_precision(const fcn8s_model* m) { return m ? m->precision : -1; }

// FCN8S_PREC_FP8_INFER calibration: the fp32 forward pass of the mode (the direct path: every FP8 layer's input is materialised), then per FP8 layer the
// maximum of |input|, accumulated on the device by an order-independent integer max (deterministic)
int fcn8s_fp8_calibrate(fcn8s_model* m, const void* images, int dtype, int N, int H, int W, int where, int reset)
{
    if (!m || !images) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_fp8_calibrate: null argument");
    if (!fp8_mode(m)) return fail(m, FCN8S_ERR_STATE, "fcn8s_fp8_calibrate: set the fp8_infer precision first (fcn8s_set_precision(m, FCN8S_PREC_FP8_INFER))");
    int rc = check_shape(m, N, H, W); if (rc) return rc;          // (a refused shape allocates nothing)
    // the amax scratch, in front of the pass: nothing on the stream touches it before launch_amax below
    if (!m->d_fp8_amax.grow(FCN8S_FP8_LAYERS * sizeof(unsigned), m->stream)) return fail(m, FCN8S_ERR_OOM, "fcn8s_fp8_calibrate: out of device memory");
    float start[FCN8S_FP8_LAYERS] = {};
    if (!reset && m->fp8_calibrated) memcpy(start, m->fp8_amax, sizeof start);
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(m->d_fp8_amax, start, sizeof start, hipMemcpyHostToDevice));
    FwdCall call; call.calibrating = true;
    rc = run_pass(m, images, dtype, nullptr, N, H, W, where, call); if (rc) return rc;
    {
        double by = 0;
        for (int L = 0; L < FCN8S_FP8_LAYERS; ++L) by += 4.0 * N * (H / kFp8InDiv[L]) * (W / kFp8InDiv[L]) * m->widths[kFp8InWidth[L]];
        ProfScope ps(m, "fp8_calibrate", 0, by);
        for (int L = 0; L < FCN8S_FP8_LAYERS; ++L) {
            const char* in = kFp8Inputs[L];
            auto it = m->acts.find(in);
            if (it == m->acts.end() || !it->second.p || m->pass.y_unwritten.count(in))
                return fail(m, FCN8S_ERR_STATE, std::string("fcn8s_fp8_calibrate: the fp32 pass did not materialise ") + in);
            const long long n = (long long)N * (H / kFp8InDiv[L]) * (W / kFp8InDiv[L]) * m->widths[kFp8InWidth[L]];
            launch_amax(it->second.p, n, m->d_fp8_amax + L, m->stream);
        }
    }
    unsigned bits[FCN8S_FP8_LAYERS];
    HIPCHK(m, hipMemcpyAsync(bits, m->d_fp8_amax, sizeof bits, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    memcpy(m->fp8_amax, bits, sizeof bits);
    m->fp8_calibrated = true;
    return FCN8S_OK;
}
int fcn8s_fp8_get_calibration(const fcn8s_model* m, float* amax, int n)
{
    if (!m || !amax || n != FCN8S_FP8_LAYERS) return FCN8S_ERR_BAD_ARG;
    if (!m->fp8_calibrated) return FCN8S_ERR_STATE;
    memcpy(amax, m->fp8_amax, sizeof m->fp8_amax);
    return FCN8S_OK;
}
int fcn8s_fp8_set_calibration(fcn8s_model* m, const float* amax, int n)
{
    if (!m || !amax) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_fp8_set_calibration: null argument");
    if (n != FCN8S_FP8_LAYERS) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_fp8_set_calibration: needs FCN8S_FP8_LAYERS (14) maxima");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(amax[i]) || amax[i] < 0.f) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_fp8_set_calibration: maxima must be finite and >= 0");
    memcpy(m->fp8_amax, amax, sizeof m->fp8_amax);
    m->fp8_calibrated = true;
    return FCN8S_OK;
}

// Options select between maintained algorithm variants (parity reports separate the Winograd round-off from the summation order
// with them); the defaults are the measured winners.  A model option drops the workspace and every cached filter bank.
static int* model_option(fcn8s_model* m, const std::string& key)
{
    if (key == "winograd_min_cin") return &m->wino_min_cin;
    if (key == "winograd_tile") return &m->wino_tile;
    if (key == "winograd_fc6") return &m->wino_fc6;
    if (key == "fc6_fft") return &m->fc6_fft;
    if (key == "fc6_fft_wgrad") return &m->fc6_fft_wgrad;
    if (key == "tconv_gemm") return &m->tconv_gemm;
    if (key == "fuse_dgrad_dout") return &m->fuse_dgrad_dout;
    if (key == "fuse_out_in") return &m->fuse_out_in;
    if (key == "bf16_gemm256") return &m->bf16_gemm256;
    if (key == "winograd_tile_hires") return &m->wino_tile_hires;
    if (key == "winograd_hires_pixels") return &m->wino_hires_pixels;
    if (key == "conv1_tiled") return &m->conv1_tiled;
    if (key == "conv1_wgrad_mfma") return &m->conv1_wgrad_mfma;
    if (key == "bf16_copy_by_transform") return &m->bf16_copy_by_transform;
    if (key == "conv1_in_transform") return &m->conv1_in_transform;
    if (key == "gemm_out_fused64") return &m->gemm_out_fused64;
    if (key == "deterministic") return &m->deterministic;
    if (key == "bf16_acts") return &m->bf16_acts;
    if (key == "bf16_rows_bn") return &m->bf16_rows_bn;
    if (key == "keep_output_gradients") return &m->keep_dy;
    if (key == "bf16_infer_copies") return &m->bf16_infer_copies;
    if (key == "bf16_fuse_pool") return &m->bf16_fuse_pool;
    return nullptr;
}
int fcn8s_set_option(fcn8s_model* m, const char* key, int64_t value)
{
    if (!key) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_option: null key");
    const std::string k = key;
    if (k == "device_bytes_live" || k == "scratch_bytes_live" || k == "op_scratch_poisoned_bytes") return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_option: '" + k + "' is read-only");
    if (!m) {
        if (k == "op_f32x3") { t_op_split = value ? 3 : 0; return FCN8S_OK; }
        if (k == "op_deterministic") { t_deterministic = value ? 1 : 0; return FCN8S_OK; }
        if (k == "op_bf16_planes") { t_op_planes = value ? 1 : 0; return FCN8S_OK; }
        if (k == "op_poison_scratch") { t_poison_scratch = value ? 1 : 0; t_scratch_poisoned_bytes = 0; return FCN8S_OK; }      // (tests: scratch_get, igemm.hip)
        if (k == "op_gemm_out_fused64") { if (value < 0 || value > 2) return fail(nullptr, FCN8S_ERR_BAD_ARG, "op_gemm_out_fused64 must be 0, 1 or 2"); t_op_fused64 = (int)value; return FCN8S_OK; }
        if (k == "op_bf16_rows_bn") { if (value != 0 && value != 64 && value != 128) return fail(nullptr, FCN8S_ERR_BAD_ARG, "op_bf16_rows_bn must be 0, 64 or 128"); t_op_rows_bn = (int)value; return FCN8S_OK; }
        if (k == "op_split_pieces") {
            if (value != 0 && value != 2 && value != 3) return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_set_option: op_split_pieces is 0, 2 or 3");
            t_op_split = (int)value; return FCN8S_OK;
        }
        return fail(nullptr, FCN8S_ERR_NOT_FOUND, "fcn8s_set_option: unknown op-context option '" + k + "' (model options need a model)");
    }
    if (k == "workspace_allocations" || k == "frozen") return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_option: '" + k + "' is read-only (the frozen state is set with fcn8s_freeze_params)");
    if (k == "comm_timeout_ms") {
        if (value < 1) return fail(m, FCN8S_ERR_BAD_ARG, "comm_timeout_ms must be >= 1");
        std::lock_guard<std::mutex> lk(m->comm_mu); m->comm_timeout_ms = value; return FCN8S_OK;
    }
    if (k == "conv1_tiled" || k == "conv1_wgrad_mfma" || k == "bf16_copy_by_transform" || k == "conv1_in_transform" || k == "deterministic" || k == "bf16_acts" || k == "bf16_rows_bn" || k == "bf16_fuse_pool" || k == "keep_output_gradients" || k == "bf16_infer_copies") {        // pick a kernel per launch: nothing cached depends on them
        *model_option(m, k) = k == "bf16_rows_bn" ? (int)value : (value ? 1 : 0);
        return FCN8S_OK;
    }
    int* slot = model_option(m, k);
    if (!slot) return fail(m, FCN8S_ERR_NOT_FOUND, "fcn8s_set_option: unknown option '" + k + "'");
    // FCN8S_PREC_BF16_TRAIN and FCN8S_PREC_FP8_INFER run without Winograd transforms whatever these two say: while such a mode is on a new value is kept
    // for the day it is left (round 5 overwrote the live slot: the value was used by nobody and lost on leaving)
    if (direct_mode(m->precision) && (k == "winograd_min_cin" || k == "winograd_fc6")) {
        if (value < 0) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_option: negative value");
        (k == "winograd_min_cin" ? m->saved_wino_min_cin : m->saved_wino_fc6) = (int)value;
        return FCN8S_OK;
    }
    if (k == "winograd_tile" && value != 2 && value != 4 && value != 6) return fail(m, FCN8S_ERR_BAD_ARG, "winograd_tile must be 2, 4 or 6");
    if (k == "winograd_tile_hires" && value != 0 && value != 2 && value != 4 && value != 6) return fail(m, FCN8S_ERR_BAD_ARG, "winograd_tile_hires must be 0, 2, 4 or 6");
    if (k == "winograd_min_cin" && value < 0) return fail(m, FCN8S_ERR_BAD_ARG, "winograd_min_cin must be >= 0 (0 = direct convolution everywhere)");
    if (k == "fuse_out_in" && (value < 0 || value > 2)) return fail(m, FCN8S_ERR_BAD_ARG, "fuse_out_in must be 0, 1 or 2");
    if (k == "fc6_fft_wgrad" && (value < 0 || value > 2)) return fail(m, FCN8S_ERR_BAD_ARG, "fc6_fft_wgrad must be 0, 1 or 2");
    if (*slot == (int)value) return FCN8S_OK;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    *slot = (k == "winograd_fc6" || k == "fc6_fft" || k == "tconv_gemm") ? (value != 0) : (int)value;
    drop_arena(m);
    drop_banks(m, true); m->u_train.clear();
    return FCN8S_OK;
}
int fcn8s_get_option(const fcn8s_model* m, const char* key, int64_t* value)
{
    if (!key || !value) return FCN8S_ERR_BAD_ARG;
    const std::string k = key;
    if (k == "device_bytes_live") { *value = g_device_bytes_live.load(); return FCN8S_OK; }      // (process-wide: with or without a model)
    if (k == "scratch_bytes_live") { *value = scratch_bytes_live(); return FCN8S_OK; }           // (process-wide too: the per-(device, stream) scratch)
    if (!m) {
        if (k == "op_f32x3") { *value = t_op_split == 3; return FCN8S_OK; }
        if (k == "op_deterministic") { *value = t_deterministic; return FCN8S_OK; }
        if (k == "op_bf16_planes") { *value = t_op_planes; return FCN8S_OK; }
        if (k == "op_poison_scratch") { *value = t_poison_scratch; return FCN8S_OK; }
        if (k == "op_scratch_poisoned_bytes") { *value = t_scratch_poisoned_bytes; return FCN8S_OK; }
        if (k == "op_gemm_out_fused64") { *value = t_op_fused64; return FCN8S_OK; }
        if (k == "op_bf16_rows_bn") { *value = t_op_rows_bn; return FCN8S_OK; }
        if (k == "op_split_pieces") { *value = t_op_split; return FCN8S_OK; }
        return FCN8S_ERR_NOT_FOUND;
    }
    if (k == "comm_timeout_ms") { *value = m->comm_timeout_ms; return FCN8S_OK; }
    if (k == "workspace_allocations") { *value = m->ws_allocs; return FCN8S_OK; }
    if (k == "frozen") { *value = m->frozen ? 1 : 0; return FCN8S_OK; }
    const int* slot = model_option(const_cast<fcn8s_model*>(m), k);
    if (!slot) return FCN8S_ERR_NOT_FOUND;
    *value = *slot;
    // (the caller's own setting, also while FCN8S_PREC_BF16_TRAIN keeps the live slots at 0)
    if (direct_mode(m->precision) && k == "winograd_min_cin" && m->saved_wino_min_cin >= 0) *value = m->saved_wino_min_cin;
    if (direct_mode(m->precision) && k == "winograd_fc6" && m->saved_wino_fc6 >= 0) *value = m->saved_wino_fc6;
    return FCN8S_OK;
}

// The model's own state (parameters, workspace, kept banks, optimizer slots, metrics) follows it across streams: the new stream waits, on the device, for
// everything the model has queued on the old one.  One event, made at the first move; the host waits only if that event cannot be made, recorded or
// waited for (a caller that destroyed the old stream too early, say): then the old stream, or failing that the device, is synchronised instead.  The
// model moves to the new stream either way, so such a mistake does not tie it to a dead handle.
int fcn8s_set_stream(fcn8s_model* m, void* s)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    hipStream_t to = (hipStream_t)s;
    if (to == m->stream) return FCN8S_OK;
    int cur = m->device; (void)hipGetDevice(&cur);           // the event belongs to the model's device, whichever one the caller has current
    if (cur != m->device) HIPCHK(m, hipSetDevice(m->device));
    hipError_t e = hipSuccess;
    if (!m->move_ev) { e = hipEventCreateWithFlags(&m->move_ev, hipEventDisableTiming); if (e != hipSuccess) m->move_ev = nullptr; }
    if (e == hipSuccess) e = hipEventRecord(m->move_ev, m->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(to, m->move_ev, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        e = hipStreamSynchronize(m->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); e = hipDeviceSynchronize(); }
    }
    m->streams_seen.insert(m->stream);
    m->stream = to;
    if (cur != m->device) (void)hipSetDevice(cur);
    HIPCHK(m, e);                                            // (only if the device itself could not be synchronised)
    return FCN8S_OK;
}
int fcn8s_synchronize(fcn8s_model* m) { if (!m) return FCN8S_ERR_BAD_ARG; HIPCHK(m, hipStreamSynchronize(m->stream)); return FCN8S_OK; }

int fcn8s_num_params(const fcn8s_model* m) { return m ? (int)m->params.size() : 0; }
int fcn8s_param_info(const fcn8s_model* m, int i, const char** name, int32_t* ndim, int64_t shape[4], int64_t* off)
{
    if (!m || i < 0 || i >= (int)m->params.size()) return FCN8S_ERR_BAD_ARG;
    const ParamInfo& p = m->params[i];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = p.ndim;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    if (off) *off = (int64_t)p.offset;
    return FCN8S_OK;
}
int fcn8s_param_index(const fcn8s_model* m, const char* name)
{
    if (!m || !name) return -1;
    auto it = m->index.find(name);
    return it == m->index.end() ? -1 : it->second;
}
static int xfer_named(fcn8s_model* m, float* base, const char* name, void* host, size_t n, bool to_dev)
{
    if (!m || !name || !host) return fail(m, FCN8S_ERR_BAD_ARG, "null argument");
    const int i = fcn8s_param_index(m, name);
    if (i < 0) return fail(m, FCN8S_ERR_NOT_FOUND, std::string("unknown variable '") + name + "'");
    const ParamInfo& p = m->params[i];
    if (n != p.numel) return fail(m, FCN8S_ERR_SHAPE, std::string("variable '") + name + "' has " + std::to_string(p.numel) + " elements, got " + std::to_string(n));
    if (base == m->d_grads) { int rcw = fcn8s_comm_wait(m); if (rcw) return rcw; }      // an all-reduce still rewriting the bucket in place: read behind it
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (to_dev) HIPCHK(m, hipMemcpy(base + p.offset, host, n * sizeof(float), hipMemcpyHostToDevice));
    else HIPCHK(m, hipMemcpy(host, base + p.offset, n * sizeof(float), hipMemcpyDeviceToHost));
    return FCN8S_OK;
}
int fcn8s_set_param(fcn8s_model* m, const char* name, const float* host, size_t n)
{
    if (m && m->frozen) fcn8s_freeze_params(m, 0);      // parameters are about to change: leave the frozen state
    fp8_clear_calibration(m);
    return xfer_named(m, m ? m->d_params : nullptr, name, (void*)host, n, true);
}
int fcn8s_get_param(fcn8s_model* m, const char* name, float* host, size_t n) { return xfer_named(m, m ? m->d_params : nullptr, name, host, n, false); }
int fcn8s_get_grad(fcn8s_model* m, const char* name, float* host, size_t n) { return xfer_named(m, m ? m->d_grads : nullptr, name, host, n, false); }
void* fcn8s_param_buffer(fcn8s_model* m, size_t* n) { if (!m) return nullptr; if (n) *n = m->total; return m->d_params; }
void* fcn8s_grad_buffer(fcn8s_model* m, size_t* n) { if (!m) return nullptr; if (n) *n = m->total; return m->d_grads; }
int fcn8s_num_buckets(const fcn8s_model* m) { return m ? kNumBuckets : 0; }
int fcn8s_bucket_range(const fcn8s_model* m, int b, size_t* off, size_t* n)
{
    if (!m || b < 0 || b >= kNumBuckets) return FCN8S_ERR_BAD_ARG;
    if (off) *off = m->bucket_off[b];
    if (n) *n = m->bucket_n[b];
    return FCN8S_OK;
}

int fcn8s_init_params(fcn8s_model* m, uint64_t seed)
{
    if (m && m->frozen) fcn8s_freeze_params(m, 0);      // parameters are about to change (or a training pass starts): leave the frozen state
    fp8_clear_calibration(m);
    if (!m) return FCN8S_ERR_BAD_ARG;
    HIPCHK(m, hipMemsetAsync(m->d_params, 0, m->total * sizeof(float), m->stream));
    uint32_t sid = 1000;
    for (auto& p : m->params) {
        ++sid;
        if (p.ndim == 1) continue;                                   // biases zero
        float std; int trunc = 0;
        const bool vgg = p.name.find("/filter") != std::string::npos || p.name.find("/weights") != std::string::npos;
        if (vgg) std = sqrtf(2.0f / (float)(p.shape[0] * p.shape[1] * p.shape[2]));
        else if (p.name.find("trans") != std::string::npos) { std = 0.01f; trunc = 1; }   // :160
        else { std = 0.001f; trunc = 1; }                                                     // :159
        launch_init_normal(m->d_params + p.offset, (long long)p.numel, std, trunc, seed, sid, m->stream);
    }
    HIPCHK(m, hipGetLastError());
    return FCN8S_OK;
}

int fcn8s_forward_loss(fcn8s_model* m, const void* images, int dtype, const uint8_t* labels, int N, int H, int W,
                       float keep_prob, float l2_rate, int where)
{
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_forward_loss");
    if (m && m->frozen) fcn8s_freeze_params(m, 0);      // parameters are about to change (or a training pass starts): leave the frozen state
    fp8_clear_calibration(m);
    if (!m || !images || !labels) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_forward_loss: null argument");
    if (!(keep_prob > 0.f && keep_prob <= 1.f)) return fail(m, FCN8S_ERR_BAD_ARG, "keep_prob must be in (0, 1]");
    if (m->kd_w != 0.f) {                                    // never train silently without a configured term
        if (!m->kd_probs) return fail(m, FCN8S_ERR_STATE, "fcn8s_set_soft_targets is on and no targets are bound: call fcn8s_bind_soft_targets before every training loss");
        if (m->kd_N != N || m->kd_H != H || m->kd_W != W)
            return fail(m, FCN8S_ERR_SHAPE, "the bound soft targets are for a batch of " + std::to_string(m->kd_N) + " x " + std::to_string(m->kd_H) + " x " +
                        std::to_string(m->kd_W) + ", the training loss for " + std::to_string(N) + " x " + std::to_string(H) + " x " + std::to_string(W));
    }
    FwdCall call; call.keep_prob = keep_prob; call.train = true;
    const uint8_t* lab;
    int rc = run_pass(m, images, dtype, labels, N, H, W, where, call, &lab); if (rc) return rc;
    rc = compute_loss(m, lab, l2_rate, true); if (rc) return rc;
    m->kd_probs = nullptr;                                   // a binding is consumed by exactly one training loss
    m->next_bucket = 0;
    for (int b = 0; b < kNumBuckets; ++b) m->acc_taken[b] = false;
    HIPCHK(m, hipGetLastError());
    return FCN8S_OK;
}

int fcn8s_backward_bucket(fcn8s_model* m, int bucket)
{
    if (!m || bucket < 0 || bucket >= kNumBuckets) return fail(m, FCN8S_ERR_BAD_ARG, "bad bucket");
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_backward_bucket");
    take_deferred_error(nullptr);
    int rc = do_backward_bucket(m, bucket); if (rc) { take_deferred_error(nullptr); return rc; }
    return deferred_rc(m);
}

int fcn8s_bucket_wait(fcn8s_model* m, int bucket, void* hip_stream)
{
    if (!m || bucket < 0 || bucket >= kNumBuckets) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_bucket_wait: bad bucket");
    if (!m->bucket_final[bucket] || !m->bucket_ev[bucket])
        return fail(m, FCN8S_ERR_STATE, "fcn8s_bucket_wait: the bucket's gradients are not queued yet (call fcn8s_backward_bucket(bucket) first)");
    HIPCHK(m, hipStreamWaitEvent((hipStream_t)hip_stream, m->bucket_ev[bucket], 0));
    return FCN8S_OK;
}

int fcn8s_bucket_complete_after(const fcn8s_model* m, int bucket)
{
    if (!m || bucket < 0 || bucket >= kNumBuckets) return -1;
    return bucket;                 // (kept for callers written when a bucket could become final at a later call)
}

// ---- the library's own RCCL communicator ------------------------------------------------------------------------------------------
// librccl is opened at run time (dlopen by soname): a process that already holds PyTorch-ROCm's copy gets that one, a plain C caller gets
// /opt/rocm's, and a single-GPU user of the library never loads the 570 MB of it.
namespace {
struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;                                   // (optional: absent in very old builds)
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t*) = nullptr;            // (optional)
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};
RcclApi* rccl()
{
    static RcclApi api; static std::once_flag once;
    std::call_once(once, [] {
        // FCN8S_RCCL_LIBRARY: the RCCL build to use, by path (a site's own build; the shared-memory stand-in of tests/fake_rccl) -- no fallback if it is set
        const char* forced = getenv("FCN8S_RCCL_LIBRARY");
        if (forced && *forced) api.h = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
        else for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { api.h = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (api.h) break; }
        if (!api.h) { const char* e = dlerror(); api.err = std::string("dlopen(") + (forced && *forced ? forced : "librccl.so.1") + "): " + (e ? e : "not found"); return; }
        auto sym = [&](const char* n) { void* p = dlsym(api.h, n); if (!p && api.err.empty()) api.err = std::string("librccl has no symbol ") + n; return p; };
        api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
        api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
        api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
        api.Broadcast = (decltype(api.Broadcast))sym("ncclBroadcast");
        api.GetVersion = (decltype(api.GetVersion))sym("ncclGetVersion");
        api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
        api.CommAbort = (decltype(api.CommAbort))dlsym(api.h, "ncclCommAbort");
        api.CommGetAsyncError = (decltype(api.CommGetAsyncError))dlsym(api.h, "ncclCommGetAsyncError");
    });
    return &api;
}
int rccl_fail(fcn8s_model* m, const char* what, ncclResult_t r)
{
    RcclApi* a = rccl();
    return fail(m, FCN8S_ERR_RCCL, std::string(what) + ": " + ((a->GetErrorString && r != ncclSuccess) ? a->GetErrorString(r) : a->err.c_str()));
}
#define RCCLCHK(m, call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) return rccl_fail(m, #call, r_); } while (0)

int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The communicator has failed (asynchronous RCCL error, or a collective older than comm_timeout_ms: a dead or hung peer).  ncclCommAbort makes
// RCCL's kernels leave the streams they sit on, so that neither the model's stream nor a host synchronisation waits for that peer forever.
// Caller holds comm_mu.
void comm_abort_locked(fcn8s_model* m, const std::string& why)
{
    if (m->comm_failed.load()) return;
    m->comm_error = why;
    m->comm_failed.store(true);
    RcclApi* a = rccl();
    if (m->comm) {
        if (a->CommAbort) a->CommAbort(m->comm);          // (frees the communicator like ncclCommDestroy, without waiting for its peers)
        m->comm = nullptr;
    }
    for (int b = 0; b < fcn8s_model::kCommSlots; ++b) m->comm_inflight[b].store(false);
    for (int b = 0; b < FCN8S_MAX_BUCKETS; ++b) m->comm_pending[b] = false;      // (the model's stream must not wait for events of a communicator that is gone)
}

// a collective has just been enqueued on `s` (caller holds comm_mu): the watchdog measures its age from now and learns of its completion from the event
int comm_track_locked(fcn8s_model* m, int slot, hipStream_t s)
{
    if (!m->comm_done[slot]) HIPCHK(m, hipEventCreateWithFlags(&m->comm_done[slot], hipEventDisableTiming));
    HIPCHK(m, hipEventRecord(m->comm_done[slot], s));
    m->comm_enq_ns[slot] = now_ns(); m->comm_inflight[slot].store(true);
    return FCN8S_OK;
}

void comm_watchdog(fcn8s_model* m)
{
    hipSetDevice(m->device);
    RcclApi* a = rccl();
    while (!m->comm_watch_stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
        std::lock_guard<std::mutex> lk(m->comm_mu);
        if (!m->comm || m->comm_failed.load()) continue;
        ncclResult_t async = ncclSuccess;
        if (a->CommGetAsyncError && a->CommGetAsyncError(m->comm, &async) == ncclSuccess && async != ncclSuccess && async != ncclInProgress) {
            comm_abort_locked(m, std::string("asynchronous RCCL error: ") + (a->GetErrorString ? a->GetErrorString(async) : "?") + " (communicator aborted)");
            continue;
        }
        const int64_t t = now_ns();
        for (int b = 0; b < fcn8s_model::kCommSlots; ++b) {
            if (!m->comm_inflight[b].load() || !m->comm_done[b]) continue;
            if (hipEventQuery(m->comm_done[b]) == hipSuccess) { m->comm_inflight[b].store(false); continue; }
            (void)hipGetLastError();                      // (hipErrorNotReady is not an error)
            if ((t - m->comm_enq_ns[b]) / 1000000 > m->comm_timeout_ms) {
                comm_abort_locked(m, (b == fcn8s_model::kCommMisc ? std::string("the parameter broadcast / metrics all-reduce") : "all-reduce of gradient bucket " + std::to_string(b)) +
                                     " did not complete within " + std::to_string(m->comm_timeout_ms) +
                                     " ms (option comm_timeout_ms): a peer rank is dead or hung; communicator aborted");
                break;
            }
        }
    }
}

// FCN8S_ERR_RCCL with the recorded reason once the communicator has failed
int comm_failed_rc(fcn8s_model* m, const char* where)
{
    std::lock_guard<std::mutex> lk(m->comm_mu);
    return fail(m, FCN8S_ERR_RCCL, std::string(where) + ": " + m->comm_error);
}
}  // namespace

int fcn8s_device_pci_bus_id(int device_id, char* out, size_t len)
{
    if (!out || len < 16) return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_device_pci_bus_id: need a buffer of at least 16 bytes");
    hipError_t e = hipDeviceGetPCIBusId(out, (int)len, device_id);
    if (e != hipSuccess) return fail(nullptr, FCN8S_ERR_HIP, std::string("hipDeviceGetPCIBusId: ") + hipGetErrorString(e));
    return FCN8S_OK;
}

int fcn8s_comm_unique_id(void* id_out, size_t nbytes)
{
    if (!id_out || nbytes < sizeof(ncclUniqueId)) return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_comm_unique_id: need a buffer of FCN8S_COMM_ID_BYTES bytes");
    RcclApi* a = rccl();
    if (!a->err.empty()) return rccl_fail(nullptr, "fcn8s_comm_unique_id", ncclSuccess);
    ncclUniqueId id;
    RCCLCHK(nullptr, a->GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return FCN8S_OK;
}

int fcn8s_comm_init(fcn8s_model* m, const void* unique_id, size_t nbytes, int rank, int world)
{
    if (!m || !unique_id || nbytes < sizeof(ncclUniqueId) || world < 1 || rank < 0 || rank >= world) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_comm_init: bad argument");
    if (m->comm) return fail(m, FCN8S_ERR_STATE, "fcn8s_comm_init: this model already has a communicator (fcn8s_comm_destroy first)");
    RcclApi* a = rccl();
    if (!a->err.empty()) return rccl_fail(m, "fcn8s_comm_init", ncclSuccess);
    HIPCHK(m, hipSetDevice(m->device));
    ncclUniqueId id; memcpy(&id, unique_id, sizeof id);
    if (m->comm_watch.joinable()) { m->comm_watch_stop.store(true); m->comm_watch.join(); }       // (left over from a communicator that failed)
    // the enum values this file declares for itself (ncclFloat = 7, ncclDouble = 8, ncclSum = 0, the result codes) are those of NCCL / RCCL 2.x
    { int v = 0; RCCLCHK(m, a->GetVersion(&v));
      const int major = v >= 10000 ? v / 10000 : v / 1000;       // (NCCL_VERSION_CODE: major * 10000 + minor * 100 + patch since 2.9, major * 1000 + ... before)
      if (major != 2) return fail(m, FCN8S_ERR_RCCL, "fcn8s_comm_init: librccl reports version code " + std::to_string(v) + "; this library speaks the RCCL 2.x ABI only"); }
    RCCLCHK(m, a->CommInitRank(&m->comm, world, id, rank));
    m->comm_rank = rank; m->comm_world = world;
    m->comm_failed.store(false); m->comm_error.clear();
    for (int b = 0; b < fcn8s_model::kCommSlots; ++b) m->comm_inflight[b].store(false);
    for (int b = 0; b < FCN8S_MAX_BUCKETS; ++b) m->comm_pending[b] = false;
    if (!m->comm_stream) HIPCHK(m, hipStreamCreateWithFlags(&m->comm_stream, hipStreamNonBlocking));
    if (world > 1) { m->comm_watch_stop.store(false); m->comm_watch = std::thread(comm_watchdog, m); }      // (a one-rank communicator has no peer to lose)
    return FCN8S_OK;
}

int fcn8s_comm_destroy(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    int rc = FCN8S_OK;
    if (m->comm) {
        // drain the communicator's stream -- but never wait for a peer that is gone: poll, with the watchdog's rules (asynchronous error or
        // comm_timeout_ms without progress -> ncclCommAbort).  A one-rank communicator, or RCCL without the two entry points, just synchronises.
        RcclApi* a = rccl();
        if (m->comm_stream) {
            const int64_t t0 = now_ns();
            while (hipStreamQuery(m->comm_stream) == hipErrorNotReady) {
                if (m->comm_failed.load()) break;
                if (m->comm_world > 1 && (now_ns() - t0) / 1000000 > m->comm_timeout_ms) {
                    std::lock_guard<std::mutex> lk(m->comm_mu);
                    comm_abort_locked(m, "fcn8s_comm_destroy: collectives still in flight after " + std::to_string(m->comm_timeout_ms) + " ms; communicator aborted");
                    break;
                }
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
            (void)hipGetLastError();
        }
        if (m->comm_watch.joinable()) { m->comm_watch_stop.store(true); m->comm_watch.join(); }
        std::lock_guard<std::mutex> lk(m->comm_mu);
        if (m->comm) { a->CommDestroy(m->comm); m->comm = nullptr; }
    }
    if (m->comm_watch.joinable()) { m->comm_watch_stop.store(true); m->comm_watch.join(); }
    if (m->comm_failed.load()) { rc = fail(m, FCN8S_ERR_RCCL, "fcn8s_comm_destroy: " + m->comm_error); m->comm_failed.store(false); }
    for (int b = 0; b < fcn8s_model::kCommSlots; ++b) { if (m->comm_done[b]) { hipEventDestroy(m->comm_done[b]); m->comm_done[b] = nullptr; } m->comm_inflight[b].store(false); }
    for (int b = 0; b < FCN8S_MAX_BUCKETS; ++b) m->comm_pending[b] = false;
    if (m->comm_stream) { hipStreamDestroy(m->comm_stream); m->comm_stream = nullptr; }
    m->comm_rank = 0; m->comm_world = 1;
    return rc;
}

int fcn8s_comm_info(const fcn8s_model* m, int* rank, int* world, int* rccl_version)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (rank) *rank = m->comm_rank;
    if (world) *world = (m->comm || m->comm_failed.load()) ? m->comm_world : 0;
    if (rccl_version) { *rccl_version = 0; RcclApi* a = rccl(); if (a->GetVersion) a->GetVersion(rccl_version); }
    return FCN8S_OK;
}

int fcn8s_allreduce_bucket(fcn8s_model* m, int bucket)
{
    if (!m || bucket < 0 || bucket >= kNumBuckets) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_allreduce_bucket: bad bucket");
    if (m->comm_failed.load()) return comm_failed_rc(m, "fcn8s_allreduce_bucket");
    if (!m->comm) return fail(m, FCN8S_ERR_STATE, "fcn8s_allreduce_bucket: no communicator (fcn8s_comm_init first)");
    if (!m->bucket_final[bucket]) return fail(m, FCN8S_ERR_STATE, "fcn8s_allreduce_bucket: the bucket's gradients are not queued yet (call fcn8s_backward_bucket(bucket) first)");
    if (m->comm_pending[bucket]) return fail(m, FCN8S_ERR_STATE, "fcn8s_allreduce_bucket: this bucket is already being reduced");
    HIPCHK(m, hipStreamWaitEvent(m->comm_stream, m->bucket_ev[bucket], 0));
    float* g = m->d_grads + m->bucket_off[bucket];
    std::lock_guard<std::mutex> lk(m->comm_mu);          // (the watchdog may abort the communicator: not in the middle of an enqueue)
    if (!m->comm) return fail(m, FCN8S_ERR_RCCL, "fcn8s_allreduce_bucket: " + m->comm_error);
    RCCLCHK(m, rccl()->AllReduce(g, g, m->bucket_n[bucket], ncclFloat, ncclSum, m->comm, m->comm_stream));
    { int rc = comm_track_locked(m, bucket, m->comm_stream); if (rc) return rc; }
    m->comm_pending[bucket] = true;
    return FCN8S_OK;
}

int fcn8s_comm_wait(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (m->comm_failed.load()) return comm_failed_rc(m, "fcn8s_comm_wait");
    for (int b = 0; b < kNumBuckets; ++b)
        if (m->comm_pending[b]) { HIPCHK(m, hipStreamWaitEvent(m->stream, m->comm_done[b], 0)); m->comm_pending[b] = false; }
    return FCN8S_OK;
}

namespace {
// The HOST waits until every pending all-reduce has completed -- polling, so that the watchdog's abort ends the wait -- and reports a failed communicator.
// fcn8s_apply_update calls it when the communicator has more than one rank: an update must never be applied to gradients whose exchange was aborted (the
// stream-ordered fcn8s_comm_wait alone would let the update kernel run behind an aborted all-reduce and report the failure one call too late).  What it
// costs is the host's run-ahead over the update kernel: a few microseconds of launch latency per step.
int comm_wait_host(fcn8s_model* m, const char* where)
{
    for (int b = 0; b < kNumBuckets; ++b) {
        if (!m->comm_pending[b]) continue;
        while (!m->comm_failed.load() && m->comm_done[b] && hipEventQuery(m->comm_done[b]) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(50));
        (void)hipGetLastError();
    }
    if (m->comm_failed.load()) return comm_failed_rc(m, where);
    return FCN8S_OK;
}
}  // namespace

int fcn8s_comm_broadcast_params(fcn8s_model* m, int root)
{
    if (!m || root < 0) return FCN8S_ERR_BAD_ARG;
    if (m->comm_failed.load()) return comm_failed_rc(m, "fcn8s_comm_broadcast_params");
    if (!m->comm) return fail(m, FCN8S_ERR_STATE, "fcn8s_comm_broadcast_params: no communicator (fcn8s_comm_init first)");
    if (root >= m->comm_world) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_comm_broadcast_params: root outside the communicator");
    if (m->frozen) fcn8s_freeze_params(m, 0);
    fp8_clear_calibration(m);
    std::lock_guard<std::mutex> lk(m->comm_mu);          // (the watchdog may abort the communicator: not in the middle of an enqueue)
    if (!m->comm) return fail(m, FCN8S_ERR_RCCL, "fcn8s_comm_broadcast_params: " + m->comm_error);
    RCCLCHK(m, rccl()->Broadcast(m->d_params, m->d_params, m->total, ncclFloat, root, m->comm, m->stream));
    return comm_track_locked(m, fcn8s_model::kCommMisc, m->stream);      // stream-ordered like every parameter write; a root that never sends trips the watchdog
}

int fcn8s_comm_allreduce_metrics(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (m->comm_failed.load()) return comm_failed_rc(m, "fcn8s_comm_allreduce_metrics");
    if (!m->comm) return fail(m, FCN8S_ERR_STATE, "fcn8s_comm_allreduce_metrics: no communicator (fcn8s_comm_init first)");
    // confusion counts (exact as doubles below 2^53), the sum of the per-batch losses and their count: one SUM all-reduce
    const size_t cc = (size_t)m->C * m->C, n = cc + 2;
    std::vector<int64_t> conf(cc); double ls; int64_t lc;
    int rc = fcn8s_metrics_raw(m, conf.data(), &ls, &lc); if (rc) return rc;
    std::vector<double> h(n);
    for (size_t i = 0; i < cc; ++i) h[i] = (double)conf[i];
    h[cc] = ls; h[cc + 1] = (double)lc;
    DeviceBuf<double> d;                                 // (freed on return: every path below leaves behind the stream's synchronise)
    if (!d.grow(n * sizeof(double), m->stream)) return fail(m, FCN8S_ERR_OOM, "fcn8s_comm_allreduce_metrics: out of device memory");
    hipMemcpyAsync(d, h.data(), n * sizeof(double), hipMemcpyHostToDevice, m->stream);
    ncclResult_t r = ncclSuccess; int rct = FCN8S_OK; bool gone = false;
    {
        std::lock_guard<std::mutex> lk(m->comm_mu);      // (the watchdog may abort the communicator: not in the middle of an enqueue)
        if (!m->comm) gone = true;
        else {
            r = rccl()->AllReduce(d, d, n, ncclDouble, ncclSum, m->comm, m->stream);
            if (r == ncclSuccess) rct = comm_track_locked(m, fcn8s_model::kCommMisc, m->stream);
        }
    }
    // the host needs the sums: wait for them by polling, so that a peer that never arrives ends in the watchdog's abort (which releases the stream), not in a hang
    if (!gone && r == ncclSuccess && rct == FCN8S_OK) {
        while (hipEventQuery(m->comm_done[fcn8s_model::kCommMisc]) == hipErrorNotReady && !m->comm_failed.load()) std::this_thread::sleep_for(std::chrono::microseconds(100));
        (void)hipGetLastError();
    }
    if (!gone && r == ncclSuccess && rct == FCN8S_OK && !m->comm_failed.load()) hipMemcpyAsync(h.data(), d, n * sizeof(double), hipMemcpyDeviceToHost, m->stream);
    hipStreamSynchronize(m->stream);                     // (behind a completed or aborted collective: returns)
    if (gone || m->comm_failed.load()) return comm_failed_rc(m, "fcn8s_comm_allreduce_metrics");
    if (r != ncclSuccess) return rccl_fail(m, "ncclAllReduce(metrics)", r);
    if (rct) return rct;
    for (size_t i = 0; i < cc; ++i) conf[i] = (int64_t)llround(h[i]);
    return fcn8s_metrics_set_raw(m, conf.data(), h[cc], (int64_t)llround(h[cc + 1]));
}

int fcn8s_accumulate_bucket(fcn8s_model* m, int bucket, int flush)
{
    if (!m || bucket < 0 || bucket >= kNumBuckets) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_accumulate_bucket: bad bucket");
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_accumulate_bucket");
    if (m->ema_swapped) return ema_refuse_swapped(m, "fcn8s_accumulate_bucket");
    if (!m->have_loss || !m->train_mode || bucket >= m->next_bucket || !m->bucket_final[bucket])
        return fail(m, FCN8S_ERR_STATE, "fcn8s_accumulate_bucket: the bucket's gradients are not queued yet (call fcn8s_backward_bucket(bucket) after fcn8s_forward_loss first)");
    if (m->acc_taken[bucket]) return fail(m, FCN8S_ERR_STATE, "fcn8s_accumulate_bucket: this backward pass's bucket has already been folded or flushed");
    if (m->comm_pending[bucket]) return fail(m, FCN8S_ERR_STATE, "fcn8s_accumulate_bucket: this bucket is being all-reduced");
    const size_t off = m->bucket_off[bucket]; const long long n = (long long)m->bucket_n[bucket];
    if (!flush) {
        if (!m->d_acc.grow(m->total * sizeof(float), m->stream, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, "fcn8s_accumulate_bucket: the accumulator cannot be allocated");
        const int mode = m->acc_k[bucket] ? 1 : 0;
        { ProfScope ps(m, "grad_accumulate", 0, (mode ? 12.0 : 8.0) * n); launch_grad_accumulate(m->d_acc + off, m->d_grads + off, n, mode, m->stream); }
        m->acc_k[bucket] += 1;
    } else if (m->acc_k[bucket] > 0) {
        { ProfScope ps(m, "grad_accumulate", 0, 12.0 * n); launch_grad_accumulate(m->d_grads + off, m->d_acc + off, n, 1, m->stream); }
        m->acc_k[bucket] = 0;
        mark_bucket_final(m, bucket, m->stream);          // the flush is now the last kernel that writes the bucket
    }
    m->acc_taken[bucket] = true;
    HIPCHK(m, hipGetLastError());
    return FCN8S_OK;
}

int fcn8s_accumulate_pending(const fcn8s_model* m)
{
    int k = 0;
    if (m) for (int b = 0; b < kNumBuckets; ++b) k = m->acc_k[b] > k ? m->acc_k[b] : k;
    return k;
}

int fcn8s_accumulate_discard(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    for (int b = 0; b < kNumBuckets; ++b) m->acc_k[b] = 0;
    return FCN8S_OK;
}

int fcn8s_set_grad_clip(fcn8s_model* m, float max_norm)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!(max_norm >= 0.f)) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_grad_clip: max_norm must be 0 (off) or in (0, +inf]");
    if (max_norm > 0.f && !m->upd_ws) {
        if (!m->upd_ws.grow(kUpdPartialsOff + kGradNormBlocks * sizeof(double), m->stream, nullptr, true)) return fail(m, FCN8S_ERR_OOM, "fcn8s_set_grad_clip: out of device memory");
    }
    m->max_norm = max_norm;
    return FCN8S_OK;
}

int fcn8s_get_update_stats(fcn8s_model* m, float* norm, float* clip_coef, float* scale, int64_t* skipped)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!m->last_update_clipped || !m->upd_ws)
        return fail(m, FCN8S_ERR_STATE, "fcn8s_get_update_stats: the last update ran without a clip setting (fcn8s_set_grad_clip)");
    UpdateStats st;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(&st, m->upd_ws, sizeof st, hipMemcpyDeviceToHost));
    if (norm) *norm = st.norm;
    if (clip_coef) *clip_coef = st.clip;
    if (scale) *scale = st.scale;
    if (skipped) *skipped = (int64_t)st.skipped;
    return FCN8S_OK;
}

// the shadow is there (allocated and set to theta at first use)
static int ensure_ema(fcn8s_model* m, bool copy_theta, const char* who)
{
    if (m->d_ema) return FCN8S_OK;
    if (!m->d_ema.grow(m->total * sizeof(float), m->stream, &m->ws_allocs)) return fail(m, FCN8S_ERR_OOM, std::string(who) + ": the shadow cannot be allocated");
    if (copy_theta) HIPCHK(m, hipMemcpyAsync(m->d_ema, m->d_params, m->total * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
    return FCN8S_OK;
}

int fcn8s_set_ema(fcn8s_model* m, double decay, int warmup)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!(decay >= 0.0 && decay < 1.0)) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_ema: decay must be 0 (off) or in (0, 1)");
    if (decay > 0.0) { int rc = ensure_ema(m, true, "fcn8s_set_ema"); if (rc) return rc; }
    m->ema_decay = decay; m->ema_warmup = warmup != 0;
    return FCN8S_OK;
}

int fcn8s_ema_reset(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!m->d_ema) return fail(m, FCN8S_ERR_STATE, "fcn8s_ema_reset: there is no shadow (fcn8s_set_ema)");
    if (m->ema_swapped) return ema_refuse_swapped(m, "fcn8s_ema_reset");
    HIPCHK(m, hipMemcpyAsync(m->d_ema, m->d_params, m->total * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
    return FCN8S_OK;
}

int fcn8s_ema_swap(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!m->d_ema) return fail(m, FCN8S_ERR_STATE, "fcn8s_ema_swap: there is no shadow (fcn8s_set_ema)");
    if (m->frozen) fcn8s_freeze_params(m, 0);      // the live parameters are about to change: leave the frozen state (what fcn8s_set_param does)
    fp8_clear_calibration(m);
    { ProfScope ps(m, "ema_swap", 0, 16.0 * m->total); launch_swap(m->d_params, m->d_ema, (long long)m->total, m->stream); }
    m->ema_swapped = !m->ema_swapped;
    HIPCHK(m, hipGetLastError());
    return FCN8S_OK;
}

int fcn8s_get_ema_info(const fcn8s_model* m, double* decay, int* warmup, int* has_shadow, int* swapped)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (decay) *decay = m->ema_decay;
    if (warmup) *warmup = m->ema_warmup;
    if (has_shadow) *has_shadow = m->d_ema ? 1 : 0;
    if (swapped) *swapped = m->ema_swapped ? 1 : 0;
    return FCN8S_OK;
}

int fcn8s_get_ema(fcn8s_model* m, float* host, size_t n)
{
    if (!m || !host || n != m->total) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_get_ema: null argument or size mismatch");
    if (!m->d_ema) return fail(m, FCN8S_ERR_STATE, "fcn8s_get_ema: there is no shadow (fcn8s_set_ema)");
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(host, m->d_ema, n * sizeof(float), hipMemcpyDeviceToHost));
    return FCN8S_OK;
}

int fcn8s_set_ema_state(fcn8s_model* m, const float* host, size_t n)
{
    if (!m || !host || n != m->total) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_ema_state: null argument or size mismatch");
    if (m->ema_swapped) return ema_refuse_swapped(m, "fcn8s_set_ema_state");
    int rc = ensure_ema(m, false, "fcn8s_set_ema_state"); if (rc) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(m->d_ema, host, n * sizeof(float), hipMemcpyHostToDevice));
    return FCN8S_OK;
}

int fcn8s_apply_update(fcn8s_model* m, int optimizer, float lr, float grad_scale)
{
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_apply_update");
    if (m && m->ema_swapped) return ema_refuse_swapped(m, "fcn8s_apply_update");
    if (fcn8s_accumulate_pending(m) > 0)
        return fail(m, FCN8S_ERR_STATE, "fcn8s_apply_update: micro-batches are folded and not flushed (fcn8s_accumulate_bucket(m, b, 1) on the last one, or fcn8s_accumulate_discard)");
    if (m && m->frozen) fcn8s_freeze_params(m, 0);      // parameters are about to change (or a training pass starts): leave the frozen state
    fp8_clear_calibration(m);
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (m->comm_world > 1 && (m->comm || m->comm_failed.load())) { int rch = comm_wait_host(m, "fcn8s_apply_update"); if (rch) return rch; }
    { int rcw = fcn8s_comm_wait(m); if (rcw) return rcw; }      // gradient buckets still being all-reduced by the library's own communicator
    const int64_t t = m->step + 1;
    // the clip: norm, c, s = grad_scale c and the guard's verdict stay on the device; the optimizer reads them there (no host round trip)
    const bool clip = m->max_norm > 0.f && (optimizer == FCN8S_OPT_TF_ADAM || optimizer == FCN8S_OPT_SGD_MOMENTUM || optimizer == FCN8S_OPT_NONE);
    UpdateStats* st = (UpdateStats*)m->upd_ws.get();
    if (clip) {
        ProfScope ps(m, "grad_norm", 0, 4.0 * m->total);
        launch_grad_norm(m->d_grads, (long long)m->total, grad_scale, m->max_norm, (double*)(m->upd_ws + kUpdPartialsOff), st, false, m->stream);
    }
    m->last_update_clipped = clip;
    // the average: w = 1 - d_t for the step this update makes; the update kernel folds the new theta into the shadow in its own pass
    const bool ema = m->ema_decay > 0.0 && m->d_ema;
    const float ema_w = ema ? ema_one_minus_decay(m->ema_decay, m->ema_warmup, t) : 0.f;
    if (optimizer == FCN8S_OPT_TF_ADAM || optimizer == FCN8S_OPT_SGD_MOMENTUM) {
        int rc = ensure_opt_state(m); if (rc) return rc;
        const bool adam = optimizer == FCN8S_OPT_TF_ADAM;
        UpdateArgs u = { optimizer, m->d_params, m->d_grads, m->d_m, nullptr, ema ? m->d_ema : nullptr, (long long)m->total,
                         lr, 0.9f, 0.f, 0.f, grad_scale, clip ? &st->scale : nullptr, clip ? &st->ok : nullptr, ema_w };      // SGD: lr, momentum 0.9
        if (adam) { u.v = m->d_v; u.p0 = tf_adam_lr_t(lr, 0.9f, 0.999f, t); u.p2 = 0.999f; u.p3 = 1e-8f; }                  // (p1: beta1 is 0.9 too)
        ProfScope ps(m, adam ? "adam" : "sgd_momentum", 0, ((adam ? 28.0 : 20.0) + (ema ? 8.0 : 0.0)) * m->total);
        launch_update(u, m->stream);
    } else if (optimizer != FCN8S_OPT_NONE) return fail(m, FCN8S_ERR_BAD_ARG, "unknown optimizer");
    else if (ema) {      // the caller has written theta: fold it as it stands on the stream
        ProfScope ps(m, "ema_update", 0, 12.0 * m->total);
        launch_ema_update(m->d_ema, m->d_params, (long long)m->total, ema_w, clip ? &st->ok : nullptr, m->stream);
    }
    m->step = t;
    HIPCHK(m, hipGetLastError());
    return FCN8S_OK;
}

int fcn8s_read_loss(fcn8s_model* m, float* loss_out)
{
    if (!m || !loss_out) return FCN8S_ERR_BAD_ARG;
    if (m->loss_copied) {
        HIPCHK(m, hipEventSynchronize(m->loss_ev));
        *loss_out = *m->h_loss;
        return FCN8S_OK;
    }
    HIPCHK(m, hipMemcpyAsync(loss_out, m->d_loss, sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return FCN8S_OK;
}

// the arguments of a weighted / OHEM loss (fcn8s_set_loss, fcn8s_op_softmax_xent_ex); weights on the host, or nullptr
static int check_loss_args(fcn8s_model* m, const float* w, int nw, int C, float thresh, int64_t min_kept, const char* who)
{
    if (w) {
        if (nw != C) return fail(m, FCN8S_ERR_BAD_ARG, std::string(who) + ": nweights must equal num_classes (" + std::to_string(C) + ")");
        bool any = false;
        for (int i = 0; i < nw; ++i) {
            if (!std::isfinite(w[i]) || w[i] < 0.f) return fail(m, FCN8S_ERR_BAD_ARG, std::string(who) + ": class weights must be finite and >= 0");
            any |= w[i] > 0.f;
        }
        if (!any) return fail(m, FCN8S_ERR_BAD_ARG, std::string(who) + ": class weights must not all be zero");
    }
    if (!(thresh == 0.f || (thresh > 0.f && thresh <= 1.f))) return fail(m, FCN8S_ERR_BAD_ARG, std::string(who) + ": ohem_thresh must be 0 (off) or in (0, 1]");
    if (min_kept < 0) return fail(m, FCN8S_ERR_BAD_ARG, std::string(who) + ": ohem_min_kept must be >= 0");
    return FCN8S_OK;
}

int fcn8s_set_loss(fcn8s_model* m, const float* class_weights, int nweights, float ohem_thresh, int64_t ohem_min_kept)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    int rc = check_loss_args(m, class_weights, nweights, m->C, ohem_thresh, ohem_min_kept, "fcn8s_set_loss"); if (rc) return rc;
    const int mode = ohem_thresh > 0.f ? 2 : class_weights ? 1 : 0;
    if (mode == 2 && m->focal_gamma > 0.f)
        return fail(m, FCN8S_ERR_STATE, "fcn8s_set_loss: OHEM does not combine with the focal loss (fcn8s_set_focal); switch one of them off");
    if (mode || m->bnd_R) {                                // (the boundary weighting alone runs the weighted mode: it must see ones, not the last weights)
        if (!m->d_cw.grow(64 * sizeof(float), m->stream)) return fail(m, FCN8S_ERR_OOM, "fcn8s_set_loss: out of device memory");
        std::vector<float> w(64, 0.f);
        for (int c = 0; c < m->C; ++c) w[c] = class_weights ? class_weights[c] : 1.f;
        HIPCHK(m, hipStreamSynchronize(m->stream));          // (a queued step may still read the old weights)
        HIPCHK(m, hipMemcpy(m->d_cw, w.data(), 64 * sizeof(float), hipMemcpyHostToDevice));
    }
    m->loss_mode = mode; m->ohem_thresh = ohem_thresh; m->ohem_min_kept = ohem_min_kept;
    return FCN8S_OK;
}

int fcn8s_get_loss_stats(fcn8s_model* m, int64_t* valid, int64_t* kept, float* threshold)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!m->last_loss_mode || !m->loss_ws)
        return fail(m, FCN8S_ERR_STATE, "fcn8s_get_loss_stats: the last training loss ran without a loss configuration (fcn8s_set_loss)");
    OhemState st;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(&st, m->loss_ws, sizeof st, hipMemcpyDeviceToHost));
    const bool ohem = m->last_loss_mode == 2;
    if (valid) *valid = (int64_t)st.valid;
    if (kept) *kept = (int64_t)(ohem ? st.kept : st.valid);
    if (threshold) *threshold = ohem ? st.t : 0.f;
    return FCN8S_OK;
}

// the arguments of fcn8s_set_lovasz (mask on the host, or nullptr = every class)
static int check_lovasz_args(fcn8s_model* m, float ce_weight, float lovasz_weight, int per_image, int classes_all, const uint8_t* mask, int nmask, int C)
{
    if (!std::isfinite(ce_weight) || !std::isfinite(lovasz_weight) || ce_weight < 0.f || lovasz_weight < 0.f)
        return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_lovasz: the weights must be finite and >= 0");
    if (ce_weight == 0.f && lovasz_weight == 0.f) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_lovasz: the weights must not both be 0");
    if ((per_image != 0 && per_image != 1) || (classes_all != 0 && classes_all != 1))
        return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_lovasz: per_image and classes_all must be 0 or 1");
    if (mask) {
        if (nmask != C) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_lovasz: nmask must equal num_classes (" + std::to_string(C) + ")");
        bool any = false;
        for (int i = 0; i < nmask; ++i) any |= mask[i] != 0;
        if (!any) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_lovasz: the class mask must not be all zero");
    }
    return FCN8S_OK;
}

int fcn8s_set_lovasz(fcn8s_model* m, float ce_weight, float lovasz_weight, int per_image, int classes_all, const uint8_t* class_mask, int nmask)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    int rc = check_lovasz_args(m, ce_weight, lovasz_weight, per_image, classes_all, class_mask, nmask, m->C); if (rc) return rc;
    const bool on = !(ce_weight == 1.f && lovasz_weight == 0.f);
    if (on) {
        if (!m->d_lovmask.grow(64, m->stream)) return fail(m, FCN8S_ERR_OOM, "fcn8s_set_lovasz: out of device memory");
        uint8_t h[64] = {};
        int n = 0;
        for (int c = 0; c < m->C; ++c) { h[c] = class_mask ? (class_mask[c] != 0) : 1; n += h[c]; }
        HIPCHK(m, hipStreamSynchronize(m->stream));          // (a queued step may still read the old mask)
        HIPCHK(m, hipMemcpy(m->d_lovmask, h, 64, hipMemcpyHostToDevice));
        m->lov_nmask = n;
    }
    m->lov_on = on; m->lov_ce = ce_weight; m->lov_w = on ? lovasz_weight : 0.f; m->lov_per_image = per_image; m->lov_all = classes_all;
    return FCN8S_OK;
}

int fcn8s_set_boundary_loss(fcn8s_model* m, int radius, const float* table256)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (radius == 0 && !table256) { m->bnd_R = 0; return FCN8S_OK; }          // off: the table and the codes stay where they are, unused
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_set_boundary_loss");
    if (!table256) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_boundary_loss: a radius needs its table (radius 0 with a NULL table switches the weighting off)");
    if (radius < 1 || radius > 15) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_boundary_loss: the radius must be in 1 .. 15 (a table needs its radius)");
    for (int i = 0; i < 256; ++i)
        if (!std::isfinite(table256[i]) || table256[i] < 0.f) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_boundary_loss: the table's entries must be finite and >= 0");
    if (!m->d_btab.grow(256 * sizeof(float), m->stream) || !m->d_cw.grow(64 * sizeof(float), m->stream))
        return fail(m, FCN8S_ERR_OOM, "fcn8s_set_boundary_loss: out of device memory");
    HIPCHK(m, hipStreamSynchronize(m->stream));              // (a queued step may still read the old table)
    HIPCHK(m, hipMemcpy(m->d_btab, table256, 256 * sizeof(float), hipMemcpyHostToDevice));
    if (!m->loss_mode) {                                     // no class weights of fcn8s_set_loss's: d_cw holds ones (see fcn8s_set_loss)
        std::vector<float> w(64, 0.f);
        for (int c = 0; c < m->C; ++c) w[c] = 1.f;
        HIPCHK(m, hipMemcpy(m->d_cw, w.data(), 64 * sizeof(float), hipMemcpyHostToDevice));
    }
    m->bnd_R = radius;
    return FCN8S_OK;
}

int fcn8s_get_boundary_codes(fcn8s_model* m, uint8_t* codes_out, int64_t nbytes)
{
    if (!m || !codes_out) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_get_boundary_codes: null argument");
    if (!m->bnd_last || !m->d_bcodes)
        return fail(m, FCN8S_ERR_STATE, "fcn8s_get_boundary_codes: the last training loss ran without the boundary weighting (fcn8s_set_boundary_loss)");
    const int64_t n = (int64_t)m->bnd_last;
    if (nbytes != n) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_get_boundary_codes: nbytes must equal N*H*W = " + std::to_string(n));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(codes_out, m->d_bcodes, (size_t)n, hipMemcpyDeviceToHost));
    return FCN8S_OK;
}

int fcn8s_get_loss_terms(fcn8s_model* m, float* ce, float* lovasz, float* l2)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!m->have_terms) return fail(m, FCN8S_ERR_STATE, "fcn8s_get_loss_terms: no training loss has run yet");
    float t[3];
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(t, m->d_terms, sizeof t, hipMemcpyDeviceToHost));
    if (ce) *ce = t[0];
    if (lovasz) *lovasz = t[1];
    if (l2) *l2 = t[2];
    return FCN8S_OK;
}

int fcn8s_set_soft_targets(fcn8s_model* m, float weight, float temperature, int all_pixels)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!std::isfinite(weight) || weight < 0.f) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_soft_targets: the weight must be finite and >= 0");
    if (!std::isfinite(temperature) || !(temperature > 0.f)) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_soft_targets: the temperature must be finite and > 0");
    if (all_pixels != 0 && all_pixels != 1) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_soft_targets: all_pixels must be 0 or 1");
    if (weight == 0.f) { m->kd_w = 0.f; m->kd_T = 1.f; m->kd_all = 0; m->kd_probs = nullptr; m->have_kd = false; return FCN8S_OK; }    // off: any binding is dropped
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_set_soft_targets");
    m->kd_w = weight; m->kd_T = temperature; m->kd_all = all_pixels;
    return FCN8S_OK;
}

int fcn8s_bind_soft_targets(fcn8s_model* m, const float* probs_dev, int N, int H, int W, int ncols, int64_t row_stride)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!probs_dev) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_bind_soft_targets: null argument");
    if (m->kd_w == 0.f) return fail(m, FCN8S_ERR_STATE, "fcn8s_bind_soft_targets: the soft-target term is off (fcn8s_set_soft_targets)");
    if (N <= 0 || H <= 0 || W <= 0) return fail(m, FCN8S_ERR_SHAPE, "fcn8s_bind_soft_targets: N, H and W must be positive");
    if (ncols < 1 || ncols > m->C) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_bind_soft_targets: ncols must be in 1 .. num_classes (" + std::to_string(m->C) + ")");
    if (row_stride < ncols) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_bind_soft_targets: row_stride must be >= ncols");
    if (((uintptr_t)probs_dev & 3) != 0) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_bind_soft_targets: the targets must be 4-byte aligned");
    m->kd_probs = probs_dev; m->kd_N = N; m->kd_H = H; m->kd_W = W; m->kd_K = ncols; m->kd_stride = (long long)row_stride;
    return FCN8S_OK;
}

int fcn8s_get_soft_target_term(fcn8s_model* m, float* kd)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!m->have_kd) return fail(m, FCN8S_ERR_STATE, "fcn8s_get_soft_target_term: the last training loss ran without the soft-target term");
    float t = 0.f;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(&t, m->d_terms + 3, sizeof t, hipMemcpyDeviceToHost));
    if (kd) *kd = t;
    return FCN8S_OK;
}

int fcn8s_set_entropy_term(fcn8s_model* m, float weight, int pixel_set, int ncols, int first_image)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!std::isfinite(weight)) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_entropy_term: the weight must be finite");
    if (pixel_set < 0 || pixel_set > 2) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_entropy_term: pixel_set must be 0 (unlabeled), 1 (valid) or 2 (all)");
    if (ncols < 2 || ncols > m->C) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_entropy_term: ncols must be in 2 .. num_classes (" + std::to_string(m->C) + ")");
    if (first_image < 0) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_entropy_term: first_image must be >= 0");
    if (weight == 0.f) { m->ent_w = 0.f; m->ent_set = 0; m->ent_K = 0; m->ent_first = 0; m->have_ent = false; return FCN8S_OK; }    // off
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_set_entropy_term");
    m->ent_w = weight; m->ent_set = pixel_set; m->ent_K = ncols; m->ent_first = first_image;
    return FCN8S_OK;
}

int fcn8s_get_entropy_term(fcn8s_model* m, float* term)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!m->have_ent) return fail(m, FCN8S_ERR_STATE, "fcn8s_get_entropy_term: the last training loss ran without the entropy term");
    float t = 0.f;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(&t, m->d_terms + 4, sizeof t, hipMemcpyDeviceToHost));
    if (term) *term = t;
    return FCN8S_OK;
}

int fcn8s_set_focal(fcn8s_model* m, float gamma)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (!std::isfinite(gamma) || gamma < 0.f || gamma > 8.f) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_set_focal: gamma must be 0 (off) or in (0, 8]");
    if (gamma == 0.f) { m->focal_gamma = 0.f; return FCN8S_OK; }    // off
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_set_focal");
    if (m->loss_mode == 2)
        return fail(m, FCN8S_ERR_STATE, "fcn8s_set_focal: the focal loss does not combine with OHEM (fcn8s_set_loss); switch one of them off");
    m->focal_gamma = gamma;
    return FCN8S_OK;
}

int fcn8s_train_step(fcn8s_model* m, const void* images, int dtype, const uint8_t* labels, int N, int H, int W,
                     float lr, float keep_prob, float l2_rate, int where, float* loss_out, int64_t* step_out)
{
    if (fp8_mode(m)) return fp8_refuse_training(m, "fcn8s_train_step");
    if (m && m->ema_swapped) return ema_refuse_swapped(m, "fcn8s_train_step");
    if (m && m->frozen) fcn8s_freeze_params(m, 0);      // parameters are about to change (or a training pass starts): leave the frozen state
    int rc = fcn8s_forward_loss(m, images, dtype, labels, N, H, W, keep_prob, l2_rate, where); if (rc) return rc;
    // a model with a communicator of more than one rank trains data-parallel through this entry point too: the bucket-by-bucket
    // backward pass, every bucket all-reduced as soon as it is final, 1/world in the update (a C caller must never get silently diverging replicas)
    const bool dp = (m->comm || m->comm_failed.load()) && m->comm_world > 1;
    // micro-batches folded before this call (fcn8s_accumulate_bucket): this is the last one -- every bucket is flushed in front of its exchange
    const int pending = fcn8s_accumulate_pending(m);
    for (int b = 0; b < kNumBuckets; ++b) {
        rc = fcn8s_backward_bucket(m, b); if (rc) return rc;
        if (pending) { rc = fcn8s_accumulate_bucket(m, b, 1); if (rc) return rc; }
        if (dp) { rc = fcn8s_allreduce_bucket(m, b); if (rc) return rc; }
    }
    float gscale = dp ? 1.f / (float)m->comm_world : 1.f;
    if (pending) gscale /= (float)(pending + 1);
    rc = fcn8s_apply_update(m, FCN8S_OPT_TF_ADAM, lr, gscale); if (rc) return rc;
    if (loss_out) { rc = fcn8s_read_loss(m, loss_out); if (rc) return rc; }
    if (step_out) *step_out = m->step;
    return FCN8S_OK;
}

int fcn8s_eval_step(fcn8s_model* m, const void* images, int dtype, const uint8_t* labels, int N, int H, int W,
                    float l2_rate, int where)
{
    if (!m || !images || !labels) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_eval_step: null argument");
    const uint8_t* lab;
    int rc = run_pass(m, images, dtype, labels, N, H, W, where, FwdCall{}, &lab); if (rc) return rc;
    rc = compute_loss(m, lab, l2_rate, false); if (rc) return rc;
    const long long npix = (long long)N * H * W;
    { ProfScope ps(m, "softmax_argmax", 0, (double)npix * (m->C * 4 + 8)); launch_softmax_argmax(LG(m), nullptr, m->d_pred, npix, m->C, m->stream, LGM(m), m->N); }
    launch_confusion(lab, m->d_pred, npix, m->d_conf, m->C, m->stream);
    float loss = 0.f;
    rc = fcn8s_read_loss(m, &loss); if (rc) return rc;          // tf.metrics.mean(total_loss): one sample per batch
    m->loss_sum += (double)loss; m->loss_cnt += 1;
    return FCN8S_OK;
}

int fcn8s_metrics_reset(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    HIPCHK(m, hipMemsetAsync(m->d_conf, 0, (size_t)m->C * m->C * sizeof(unsigned long long), m->stream));
    m->loss_sum = 0; m->loss_cnt = 0;
    return FCN8S_OK;
}

int fcn8s_metrics_raw(fcn8s_model* m, int64_t* conf, double* loss_sum, int64_t* loss_cnt)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    if (conf) {
        HIPCHK(m, hipMemcpyAsync(conf, m->d_conf, (size_t)m->C * m->C * sizeof(int64_t), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(m, hipStreamSynchronize(m->stream));
    }
    if (loss_sum) *loss_sum = m->loss_sum;
    if (loss_cnt) *loss_cnt = m->loss_cnt;
    return FCN8S_OK;
}

int fcn8s_metrics_set_raw(fcn8s_model* m, const int64_t* conf, double loss_sum, int64_t loss_cnt)
{
    if (!m || !conf) return FCN8S_ERR_BAD_ARG;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(m->d_conf, conf, (size_t)m->C * m->C * sizeof(int64_t), hipMemcpyHostToDevice));
    m->loss_sum = loss_sum; m->loss_cnt = loss_cnt;
    return FCN8S_OK;
}

int fcn8s_metrics_get(fcn8s_model* m, double* mean_loss, double* mean_iou, double* accuracy)
{
    return fcn8s_metrics_get_ex(m, mean_loss, mean_iou, accuracy, 0);
}

int fcn8s_metrics_get_ex(fcn8s_model* m, double* mean_loss, double* mean_iou, double* accuracy, int all_classes)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    const int C = m->C;
    std::vector<int64_t> cm((size_t)C * C);
    int rc = fcn8s_metrics_raw(m, cm.data(), nullptr, nullptr); if (rc) return rc;
    // tf.metrics.mean_iou: iou_c = diag/(row+col-diag) with zero denominators replaced by 1; mean over the classes with a non-zero
    // denominator (later TF 1.x), or -- all_classes, the TF 1.3.0 of fcn8s_tutorial.ipynb:311 -- over all C classes (an absent class counts as IoU 0)
    double iou_sum = 0, tot = 0, diag = 0; int valid = 0;
    for (int c = 0; c < C; ++c) {
        double row = 0, col = 0;
        for (int k = 0; k < C; ++k) { row += (double)cm[(size_t)c * C + k]; col += (double)cm[(size_t)k * C + c]; }
        const double d = (double)cm[(size_t)c * C + c];
        const double den = row + col - d;
        if (den > 0) { iou_sum += d / den; ++valid; }
        tot += row; diag += d;
    }
    if (mean_loss) *mean_loss = m->loss_cnt > 0 ? m->loss_sum / (double)m->loss_cnt : 0.0;
    if (mean_iou) *mean_iou = all_classes ? iou_sum / C : (valid > 0 ? iou_sum / valid : 0.0);
    if (accuracy) *accuracy = tot > 0 ? diag / tot : 0.0;
    return FCN8S_OK;
}

int fcn8s_predict(fcn8s_model* m, const void* images, int dtype, int N, int H, int W, int argmax, void* out, int where)
{
    if (!m || !images || !out) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict: null argument");
    int rc = run_pass(m, images, dtype, nullptr, N, H, W, where, FwdCall{}); if (rc) return rc;
    const long long npix = (long long)N * H * W;
    if (where == FCN8S_DEVICE) {
        ProfScope ps(m, "softmax_argmax", 0, (double)npix * (m->C * 4 + 8));
        if (argmax) launch_softmax_argmax(LG(m), nullptr, (long long*)out, npix, m->C, m->stream, LGM(m), m->N);
        else launch_softmax_argmax(LG(m), (float*)out, nullptr, npix, m->C, m->stream, LGM(m), m->N);
        HIPCHK(m, hipGetLastError());
        return FCN8S_OK;
    }
    if (argmax) {
        launch_softmax_argmax(LG(m), nullptr, m->d_pred, npix, m->C, m->stream, LGM(m), m->N);
        HIPCHK(m, hipMemcpyAsync(out, m->d_pred, npix * sizeof(long long), hipMemcpyDeviceToHost, m->stream));
    } else {
        launch_softmax_argmax(LG(m), m->d_softmax, nullptr, npix, m->C, m->stream, LGM(m), m->N);
        HIPCHK(m, hipMemcpyAsync(out, m->d_softmax, npix * m->C * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return FCN8S_OK;
}

// ---- multi-scale / flip inference (test-time augmentation) ----------------------------------------------------------------------
// P = nscales x (1 + flip) passes, in the order (scale 0, scale 0 mirrored, scale 1, ...).  Pass k: the image resized to Hs x Ws (cv2 INTER_LINEAR,
// bit-exact with resample_u8), mirrored, preprocessed and zero padded to Hp x Wp = 32 ceil(Hs / 32) x 32 ceil(Ws / 32) by tta_input straight into x0;
// the predict forward; tta_accumulate reads the logits over [0,Hs)x[0,Ws) through the PixMap, un-mirrors, resizes them to H x W (half-pixel
// bilinear), softmaxes and sums in pass order; the last pass writes the mean (or its argmax).  All passes share one arena sized for the largest,
// and the call runs with frozen parameters (FrozenForCall).
int fcn8s_predict_tta(fcn8s_model* m, const void* images, int dtype, int N, int H, int W, const float* scales, int nscales, int flip,
                      int argmax, void* out, int where)
{
    if (!m || !images || !out || !scales) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_tta: null argument");
    int rc = check_predict_args(m, "fcn8s_predict_tta", dtype, where); if (rc) return rc;
    if (nscales < 1 || nscales > 8) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_tta: between 1 and 8 scales");
    rc = check_predict_shape(m, "fcn8s_predict_tta", N, H, W); if (rc) return rc;
    int hs[8], ws[8], hp[8], wp[8];
    for (int k = 0; k < nscales; ++k) {
        const float sc = scales[k];
        if (!std::isfinite(sc) || !(sc > 0.f) || sc > 4.f) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_tta: every scale must lie in (0, 4]");
        hs[k] = std::max(1, (int)std::floor((double)H * (double)sc + 0.5));
        ws[k] = std::max(1, (int)std::floor((double)W * (double)sc + 0.5));
        hp[k] = (hs[k] + 31) / 32 * 32; wp[k] = (ws[k] + 31) / 32 * 32;
        if (dtype == FCN8S_IMG_F32 && (hs[k] != H || ws[k] != W))
            return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_tta: float32 images are taken only when no pass resizes them (every scale maps H x W to itself)");
        rc = check_padded_shape(m, "fcn8s_predict_tta", "a pass's", N, hp[k], wp[k]); if (rc) return rc;
    }
    flip = flip ? 1 : 0;
    // the identity case is fcn8s_predict itself (bit for bit)
    if (nscales == 1 && !flip && hs[0] == H && ws[0] == W && hp[0] == H && wp[0] == W) return fcn8s_predict(m, images, dtype, N, H, W, argmax, out, where);
    const int P = nscales * (1 + flip), C = m->C;
    size_t need = 0;
    for (int k = 0; k < nscales; ++k) { WsPlan pl; plan_workspace(m, N, hp[k], wp[k], pl); need = std::max(need, pl.bytes); }
    if (fp8_mode(m)) {                    // fp8_infer: every e4m3 copy sized for the largest pass up front (no reallocation between passes)
        for (const Q8Spec& q : q8_specs(m)) {
            size_t mx = 0;
            for (int k = 0; k < nscales; ++k) mx = std::max(mx, q8_bytes(N, hp[k] / q.div, wp[k] / q.div, q.C, q.K));
            if (!q8_grow(m, q.key, mx, m->stream)) return fail(m, FCN8S_ERR_OOM, "fcn8s_predict_tta: hipMalloc of an e4m3 copy failed");
        }
    }
    // scratch: the staged images (host input), the accumulator (P > 1), the staged output (host output)
    const size_t npix = (size_t)N * H * W, eb = dtype == FCN8S_IMG_U8 ? 1 : 4;
    Scratch sc{m->tta_buf}; PredictIo io(m, sc, where);
    io.input(images, npix * 3 * eb);
    const Scratch::Item i_acc = sc.take(P > 1 ? npix * C * sizeof(float) : 0);
    const int o = io.output(out, argmax ? npix * sizeof(long long) : npix * C * sizeof(float));
    if (!sc.grow(m)) return fail(m, FCN8S_ERR_OOM, "fcn8s_predict_tta: its scratch cannot be allocated");
    rc = io.stage(); if (rc) return rc;
    hipStream_t s = m->stream;
    const void* img = io.images_dev();
    float* acc = sc.ptr<float>(i_acc); float* sm; long long* am;
    io.split(o, argmax != 0, &sm, &am);
    FwdCall call; call.x0_written = true;
    FrozenForCall frozen(m);
    for (int pi = 0; pi < P; ++pi) {
        const int k = pi / (1 + flip), f = flip ? pi % 2 : 0;
        rc = ensure_workspace_at_least(m, N, hp[k], wp[k], need); if (rc) return rc;
        { ProfScope ps(m, "tta_input", 0, (double)npix * 3 * eb + 16.0 * N * hp[k] * wp[k]);
          launch_tta_input(img, dtype, N, H, W, hs[k], ws[k], hp[k], wp[k], f, A(m, "x0"), s); }
        rc = run_forward(m, img, dtype, call); if (rc) return rc;
        const bool first = pi == 0, last = pi == P - 1;
        // algorithmic bytes: the valid logits once, the accumulator read (not first) / written (not last), the result (last)
        const double by = 4.0 * N * hs[k] * ws[k] * C + (first ? 0.0 : 4.0 * npix * C) + (last ? 0.0 : 4.0 * npix * C) + (last ? (argmax ? 8.0 * npix : 4.0 * npix * C) : 0.0);
        { ProfScope ps(m, "tta_accumulate", 0, by);
          launch_tta_accumulate(LG(m), logits_map(m, hp[k], wp[k]), N, hs[k], ws[k], f, C, H, W, acc, first, last, P, sm, am, s); }
    }
    HIPCHK(m, hipGetLastError());
    return io.copy_out();
}

// ---- Monte-Carlo dropout inference (definition: fcn8s_hip.h at fcn8s_predict_mc) --------------------------------------------------
// One prediction forward whose encoder and skip heads run once and whose fc6 -> fc7 -> decoder part runs `samples` times with dropout on (forward()'s
// McLoop); behind each sample mc_accumulate folds its logits, read over [0,H)x[0,W) through the PixMap, into the running sums, and the last sample
// writes the outputs.  The image is padded to multiples of 32 by tta_input (a shape that needs no padding goes through the preprocess kernel, as
// fcn8s_predict).  The call runs with frozen parameters (FrozenForCall): every sample after the first reuses fc6's / fc7's banks.
int fcn8s_predict_mc(fcn8s_model* m, const void* images, int dtype, int N, int H, int W, int samples, float keep_prob, int64_t sample_offset,
                     int argmax, void* out, float* entropy_out, float* mi_out, int where)
{
    if (!m || !images) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_mc: null argument");
    if (!out && !entropy_out && !mi_out) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_mc: no output was asked for (out, entropy_out and mi_out are all null)");
    int rc = check_predict_args(m, "fcn8s_predict_mc", dtype, where); if (rc) return rc;
    if (samples < 1 || samples > FCN8S_MC_MAX_SAMPLES) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_mc: between 1 and 256 samples");
    if (!(keep_prob > 0.f) || !(keep_prob <= 1.f)) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_mc: keep_prob must lie in (0, 1]");
    if (sample_offset < 0 || sample_offset + samples > (int64_t)1 << 30)
        return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_mc: sample_offset must be >= 0 with sample_offset + samples <= 2^30 (the counter streams 0x80000000 + 2 (offset + s) of the masks)");
    if (fp8_mode(m)) return fail(m, FCN8S_ERR_STATE, "fcn8s_predict_mc: fp8_infer has no Monte-Carlo dropout -- its fc6 / fc7 kernels have no dropout epilogue; set another precision for the call");
    rc = check_predict_shape(m, "fcn8s_predict_mc", N, H, W); if (rc) return rc;
    const int Hp = (H + 31) / 32 * 32, Wp = (W + 31) / 32 * 32, C = m->C, S = samples;
    rc = check_padded_shape(m, "fcn8s_predict_mc", "the", N, Hp, Wp); if (rc) return rc;
    rc = ensure_workspace(m, N, Hp, Wp); if (rc) return rc;
    // scratch: the staged images (host input), the two accumulators (S > 1), the staged outputs (host output)
    const size_t npix = (size_t)N * H * W, eb = dtype == FCN8S_IMG_U8 ? 1 : 4;
    Scratch sc{m->mc_buf}; PredictIo io(m, sc, where);
    io.input(images, npix * 3 * eb);
    const Scratch::Item i_acc = sc.take(S > 1 ? npix * C * sizeof(float) : 0), i_eacc = sc.take(S > 1 ? npix * sizeof(float) : 0);
    const int o_out = io.output(out, argmax ? npix * sizeof(long long) : npix * C * sizeof(float));
    const int o_ent = io.output(entropy_out, npix * sizeof(float)), o_mi = io.output(mi_out, npix * sizeof(float));
    if (!sc.grow(m)) return fail(m, FCN8S_ERR_OOM, "fcn8s_predict_mc: its scratch cannot be allocated");
    rc = io.stage(); if (rc) return rc;
    hipStream_t s = m->stream;
    const void* img = io.images_dev();
    float *acc = sc.ptr<float>(i_acc), *eacc = sc.ptr<float>(i_eacc), *d_ent = (float*)io.dev(o_ent), *d_mi = (float*)io.dev(o_mi), *sm; long long* am;
    io.split(o_out, argmax != 0, &sm, &am);
    McLoop mc; mc.samples = S; mc.stream_base = 0x80000000u + 2u * (uint32_t)sample_offset;
    FwdCall call; call.keep_prob = keep_prob; call.mc = &mc; call.x0_written = Hp != H || Wp != W;
    mc.after_sample = [&](int k) {
        const bool first = k == 0, last = k == S - 1;
        // algorithmic bytes: the valid logits once, both accumulators read (not first) / written (not last), the outputs (last)
        const double by = 4.0 * npix * C + ((first ? 0.0 : 1.0) + (last ? 0.0 : 1.0)) * 4.0 * npix * (C + 1) +
                          (last ? (sm ? 4.0 * npix * C : 0.0) + (am ? 8.0 * npix : 0.0) + (d_ent ? 4.0 * npix : 0.0) + (d_mi ? 4.0 * npix : 0.0) : 0.0);
        ProfScope ps(m, "mc_accumulate", 0, by);
        launch_mc_accumulate(LG(m), logits_map(m, Hp, Wp), N, H, W, C, acc, eacc, first, last, S, sm, am, d_ent, d_mi, s);
    };
    FrozenForCall frozen(m);
    if (call.x0_written) {
        ProfScope ps(m, "tta_input", 0, (double)npix * 3 * eb + 16.0 * N * Hp * Wp);
        launch_tta_input(img, dtype, N, H, W, H, W, Hp, Wp, 0, A(m, "x0"), s);
    }
    rc = run_forward(m, img, dtype, call); if (rc) return rc;
    HIPCHK(m, hipGetLastError());
    return io.copy_out();
}

// ---- mean-field CRF refinement (definition: fcn8s_hip.h at fcn8s_crf_params) ------------------------------------------------------
// the field of p that lies outside its range, or nullptr
static const char* crf_bad_field(const fcn8s_crf_params* p)
{
    if (p->iterations < 0 || p->iterations > 32) return "iterations (0..32)";
    if (p->radius < 1 || p->radius > 7) return "radius (1..7)";
    if (p->dilation < 1 || p->dilation > 8) return "dilation (1..8)";
    if (!std::isfinite(p->w_appearance) || !(p->w_appearance >= 0.f)) return "w_appearance (finite, >= 0)";
    if (!std::isfinite(p->w_smooth) || !(p->w_smooth >= 0.f)) return "w_smooth (finite, >= 0)";
    if (!std::isfinite(p->theta_alpha) || !(p->theta_alpha > 0.f)) return "theta_alpha (finite, > 0)";
    if (!std::isfinite(p->theta_beta) || !(p->theta_beta > 0.f)) return "theta_beta (finite, > 0)";
    if (!std::isfinite(p->theta_gamma) || !(p->theta_gamma > 0.f)) return "theta_gamma (finite, > 0)";
    return nullptr;
}
// iterations >= 1 updates from prob; update t writes q_out when it is the last and q_out is given, else work half (t & 1); m (may be nullptr): profile group
static void crf_run(fcn8s_model* m, hipStream_t s, const float* prob, const uint8_t* images, int N, int H, int W, int C, const fcn8s_crf_params* p,
                    float* work, float* q_out, long long* argmax_out)
{
    const size_t n = (size_t)N * H * W * C;
    const long long npix = (long long)N * H * W;
    const double taps = (double)(2 * p->radius + 1) * (2 * p->radius + 1) - 1;
    const float* src = prob;
    for (int t = 1; t <= p->iterations; ++t) {
        const bool last = t == p->iterations;
        float* dst = last && q_out ? q_out : work + (size_t)(t & 1) * n;
        // algorithmic: read Q, read P, write Q, read the image (+ the argmax); 2 flops per FMA of the two messages
        const double by = (double)npix * (12.0 * C + 3.0) + (last && argmax_out ? 8.0 * npix : 0.0), fl = (double)npix * taps * 4.0 * C;
        auto launch = [&] {
            launch_crf_meanfield(src, prob, images, N, H, W, C, p->radius, p->dilation, p->w_appearance, p->w_smooth, p->theta_alpha, p->theta_beta,
                                 p->theta_gamma, dst, last ? argmax_out : nullptr, s);
        };
        { ProfScope ps(m, "crf_meanfield", fl, by); launch(); }
        src = dst;
    }
}

int fcn8s_predict_crf(fcn8s_model* m, const void* images, int dtype, int N, int H, int W, const float* scales, int nscales, int flip,
                      const fcn8s_crf_params* crf, int argmax, void* out, int where)
{
    if (!m) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_crf: null argument");
    if (crf) { const char* bad = crf_bad_field(crf); if (bad) return fail(m, FCN8S_ERR_BAD_ARG, std::string("fcn8s_predict_crf: crf_params.") + bad + " is out of range"); }
    if (!crf || crf->iterations == 0) return fcn8s_predict_tta(m, images, dtype, N, H, W, scales, nscales, flip, argmax, out, where);
    if (!images || !out || !scales) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_crf: null argument");
    if (dtype != FCN8S_IMG_U8) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_predict_crf: the mean field (iterations > 0) reads the colours of uint8 images; float32 images are not taken");
    int rc = check_predict_args(m, "fcn8s_predict_crf", dtype, where); if (rc) return rc;
    rc = check_predict_shape(m, "fcn8s_predict_crf", N, H, W); if (rc) return rc;
    const int C = m->C;
    if (!crf_shape_supported(C, crf->radius)) return fail(m, FCN8S_ERR_SHAPE, "fcn8s_predict_crf: this many classes do not fit the mean field's LDS tile at this radius");
    // scratch: the staged images (host input), the mean softmax, the two mean-field buffers, the staged output (host output)
    const size_t npix = (size_t)N * H * W, qb = npix * C * sizeof(float);
    Scratch sc{m->crf_buf}; PredictIo io(m, sc, where);
    io.input(images, npix * 3);
    const Scratch::Item i_prob = sc.take(qb), i_work = sc.take(qb);          // work: crf_run's two halves of N H W C floats, ...
    sc.take(qb);                                                             // ... the second one's room
    const int o = io.output(out, argmax ? npix * sizeof(long long) : qb);
    if (!sc.grow(m)) return fail(m, FCN8S_ERR_OOM, "fcn8s_predict_crf: its scratch cannot be allocated");
    rc = io.stage(); if (rc) return rc;
    const uint8_t* img = (const uint8_t*)io.images_dev();
    float *prob = sc.ptr<float>(i_prob), *sm; long long* am;
    io.split(o, argmax != 0, &sm, &am);
    rc = fcn8s_predict_tta(m, img, dtype, N, H, W, scales, nscales, flip, 0, prob, FCN8S_DEVICE); if (rc) return rc;
    take_deferred_error(nullptr);
    // argmax: Q^T goes to a work half; softmax: the last update writes it where it is wanted
    crf_run(m, m->stream, prob, img, N, H, W, C, crf, sc.ptr<float>(i_work), sm, am);
    rc = deferred_rc(m); if (rc) return rc;
    HIPCHK(m, hipGetLastError());
    return io.copy_out();
}

// ---- asynchronous host boundary ------------------------------------------------------------------
int fcn8s_stage_inputs(fcn8s_model* m, int slot, const void* images, int dtype, const uint8_t* label_ids, int N, int H, int W,
                       void** images_dev, uint8_t** labels_dev)
{
    if (!m || !images || slot < 0 || slot >= FCN8S_NUM_STAGE_SLOTS || N <= 0 || H <= 0 || W <= 0) return fail(m, FCN8S_ERR_BAD_ARG, "fcn8s_stage_inputs: bad argument");
    HIPCHK(m, hipSetDevice(m->device));                  // may be called from a feeder thread
    if (!m->copy_stream) HIPCHK(m, hipStreamCreateWithFlags(&m->copy_stream, hipStreamNonBlocking));
    fcn8s_model::StageSlot& sl = m->slots[slot];
    const size_t npix = (size_t)N * H * W, ib = npix * 3 * (dtype == FCN8S_IMG_U8 ? 1 : 4), lb = label_ids ? npix : 0;
    if (!sl.ready) { HIPCHK(m, hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming)); HIPCHK(m, hipEventCreateWithFlags(&sl.consumed, hipEventDisableTiming)); }
    if (sl.used) HIPCHK(m, hipEventSynchronize(sl.ready));        // the previous copy out of this slot's pinned buffers has finished
    // (a pair that grows: the step that last read the device half has finished with it -- `consumed` -- before the pair is freed)
    if ((sl.d_img.bytes() < ib || sl.d_lab.bytes() < lb) && sl.used) HIPCHK(m, hipEventSynchronize(sl.consumed));
    if (!sl.h_img.grow(ib, m->copy_stream) || !sl.d_img.grow(ib, m->copy_stream) || (lb && (!sl.h_lab.grow(lb, m->copy_stream) || !sl.d_lab.grow(lb, m->copy_stream))))
        return fail(m, FCN8S_ERR_OOM, "fcn8s_stage_inputs: the slot's buffers cannot be allocated");
    memcpy(sl.h_img, images, ib);                         // pageable -> pinned on this (feeder) thread
    if (lb) memcpy(sl.h_lab, label_ids, lb);
    if (sl.used) HIPCHK(m, hipStreamWaitEvent(m->copy_stream, sl.consumed, 0));   // the step that last read this slot's device buffers
    HIPCHK(m, hipMemcpyAsync(sl.d_img, sl.h_img, ib, hipMemcpyHostToDevice, m->copy_stream));
    if (lb) HIPCHK(m, hipMemcpyAsync(sl.d_lab, sl.h_lab, lb, hipMemcpyHostToDevice, m->copy_stream));
    HIPCHK(m, hipEventRecord(sl.ready, m->copy_stream));
    sl.used = true;
    if (images_dev) *images_dev = sl.d_img;
    if (labels_dev) *labels_dev = lb ? sl.d_lab.get() : nullptr;
    return FCN8S_OK;
}
int fcn8s_stage_wait(fcn8s_model* m, int slot)
{
    if (!m || slot < 0 || slot >= FCN8S_NUM_STAGE_SLOTS || !m->slots[slot].used) return fail(m, FCN8S_ERR_STATE, "fcn8s_stage_wait: nothing staged in this slot");
    HIPCHK(m, hipStreamWaitEvent(m->stream, m->slots[slot].ready, 0));
    return FCN8S_OK;
}
int fcn8s_stage_release(fcn8s_model* m, int slot)
{
    if (!m || slot < 0 || slot >= FCN8S_NUM_STAGE_SLOTS || !m->slots[slot].used) return fail(m, FCN8S_ERR_STATE, "fcn8s_stage_release: nothing staged in this slot");
    HIPCHK(m, hipEventRecord(m->slots[slot].consumed, m->stream));
    return FCN8S_OK;
}

int64_t fcn8s_global_step(const fcn8s_model* m) { return m ? m->step : -1; }
int fcn8s_set_global_step(fcn8s_model* m, int64_t s) { if (!m || s < 0) return FCN8S_ERR_BAD_ARG; m->step = s; return FCN8S_OK; }

int fcn8s_get_opt_state(fcn8s_model* m, float* hm, float* hv, size_t n)
{
    if (!m || n != m->total) return fail(m, FCN8S_ERR_BAD_ARG, "optimizer state size mismatch");
    int rc = ensure_opt_state(m); if (rc) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (hm) HIPCHK(m, hipMemcpy(hm, m->d_m, n * sizeof(float), hipMemcpyDeviceToHost));
    if (hv) HIPCHK(m, hipMemcpy(hv, m->d_v, n * sizeof(float), hipMemcpyDeviceToHost));
    return FCN8S_OK;
}
int fcn8s_set_opt_state(fcn8s_model* m, const float* hm, const float* hv, size_t n)
{
    if (!m || n != m->total) return fail(m, FCN8S_ERR_BAD_ARG, "optimizer state size mismatch");
    int rc = ensure_opt_state(m); if (rc) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (hm) HIPCHK(m, hipMemcpy(m->d_m, hm, n * sizeof(float), hipMemcpyHostToDevice));
    if (hv) HIPCHK(m, hipMemcpy(m->d_v, hv, n * sizeof(float), hipMemcpyHostToDevice));
    return FCN8S_OK;
}

int fcn8s_get_activation(fcn8s_model* m, const char* name, float* host, size_t n)
{
    if (!m || !name || !host) return FCN8S_ERR_BAD_ARG;
    if (!m->have_forward) return fail(m, FCN8S_ERR_STATE, "no forward pass has been run");
    if (strncmp(name, "dy:", 3) == 0) {      // a layer's output gradient as the last backward pass handed it to the weight gradient (option "keep_output_gradients")
        auto k = m->kept_dy.find(name + 3);
        if (k == m->kept_dy.end() || !k->second.p || !k->second.n)
            return fail(m, FCN8S_ERR_STATE, std::string("no fp32 output gradient of '") + (name + 3) + "' was kept: set option \"keep_output_gradients\" before the backward pass (bf16_train: with \"bf16_acts\" = 0; "
                                            "a gradient handed on as routing bytes, as a Winograd-domain image or as a bf16 copy only has no fp32 tensor)");
        if (n != k->second.n) return fail(m, FCN8S_ERR_SHAPE, std::string("output gradient of '") + (name + 3) + "' has " + std::to_string(k->second.n) + " elements");
        HIPCHK(m, hipDeviceSynchronize());
        HIPCHK(m, hipMemcpy(host, k->second.p, n * sizeof(float), hipMemcpyDeviceToHost));
        return FCN8S_OK;
    }
    if (strncmp(name, "q8:", 3) == 0) {      // FCN8S_PREC_FP8_INFER: a layer's e4m3 input copy of the last pass, dequantized (2^ex code: exact in fp32) as [N,H,W,Cin]
        auto k = m->q8.find(name + 3);
        if (!fp8_mode(m) || k == m->q8.end() || !k->second.p || !m->pass.q8_filled.count(name + 3) || fp8_layer(name + 3) < 0)
            return fail(m, FCN8S_ERR_STATE, std::string("no e4m3 input copy of '") + (name + 3) + "': run an fp8_infer evaluation / prediction first (FP8 layers: conv1_2 .. conv5_3, fc6, fc7)");
        const Q8Buf& b = k->second;
        const size_t need = (size_t)b.N * b.H * b.W * b.C;
        if (n != need) return fail(m, FCN8S_ERR_SHAPE, std::string("e4m3 copy of '") + (name + 3) + "' has " + std::to_string(need) + " elements");
        std::vector<unsigned char> raw((size_t)b.ps * (b.C / 64));
        HIPCHK(m, hipStreamSynchronize(m->stream));
        HIPCHK(m, hipMemcpy(raw.data(), b.p, raw.size(), hipMemcpyDeviceToHost));
        float lut[256];
        for (int c = 0; c < 256; ++c) {
            const int e = (c >> 3) & 15, mt = c & 7;
            const double v = (e == 15 && mt == 7) ? NAN : (e ? ldexp(1.0 + mt / 8.0, e - 7) : ldexp((double)mt, -9));
            lut[c] = (float)ldexp((c & 128) ? -v : v, b.ex);
        }
        const int Hp = b.H + 2 * b.pad, Wq = b.W + 2 * b.pad;
        for (int nn = 0; nn < b.N; ++nn)
            for (int y = 0; y < b.H; ++y)
                for (int x = 0; x < b.W; ++x) {
                    const long long q = ((long long)nn * Hp + y + b.pad) * Wq + x + b.pad;
                    float* dst = host + (((size_t)nn * b.H + y) * b.W + x) * b.C;
                    for (int c = 0; c < b.C; ++c) dst[c] = lut[raw[(size_t)(c >> 6) * b.ps + q * 64 + (c & 63)]];
                }
        return FCN8S_OK;
    }
    auto it = m->acts.find(name);
    if (it == m->acts.end()) return fail(m, FCN8S_ERR_NOT_FOUND, std::string("unknown activation '") + name + "'");
    if (std::string(name) == "logits" && !m->logits_nhwc_valid && m->logits_b) {      // kept in the blocked GEMM layout: convert for the caller
        launch_unblock_logits(m->logits_b, it->second.p, m->pm, m->N, m->C, m->stream);
        m->logits_nhwc_valid = true;
    }
    if (n != it->second.n) return fail(m, FCN8S_ERR_SHAPE, std::string("activation '") + name + "' has " + std::to_string(it->second.n) + " elements");
    if (m->pass.y_unwritten.count(name))
        return fail(m, FCN8S_ERR_STATE, std::string("activation '") + name + "' was not materialised by the last forward pass: " +
                                        (fp8_mode(m) ? std::string("fp8_infer keeps it only as its consumer's e4m3 copy (fcn8s_get_activation(m, \"q8:<consumer>\", ...))") :
                                         bf16_train_mode(m) ? "bf16_train keeps a conv -> conv activation only as the consumer's padded bf16 copy (option \"bf16_acts\" = 0 keeps the fp32 tensor too)" :
                                         std::string(name) == "conv1_1" ? "conv1_2's input transform evaluated it on its own patches (option \"conv1_in_transform\" = 0 keeps it)"
                                                                        : "its output transform wrote the next conv's transformed input directly (option \"fuse_out_in\" = 0 keeps it)"));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(host, it->second.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return FCN8S_OK;
}

int fcn8s_get_relu_record(fcn8s_model* m, const char* layer, unsigned char* host, size_t n)
{
    if (!m || !layer || !host) return FCN8S_ERR_BAD_ARG;
    if (!m->have_forward || !m->train_mode) return fail(m, FCN8S_ERR_STATE, "fcn8s_get_relu_record: no training forward pass has been run");
    const Layer* L = find_layer(m, layer);
    if (!L || !in_block_next(m->layers, *L))
        return fail(m, FCN8S_ERR_NOT_FOUND, std::string("fcn8s_get_relu_record: '") + layer + "' is not a conv that feeds another conv");
    if (!L->rb || !m->pass.rbits_ok.count(layer))
        return fail(m, FCN8S_ERR_STATE, std::string("fcn8s_get_relu_record: the last forward pass kept no ReLU record of '") + layer + "' (the backward pass reads the activation itself)");
    const int H = L->h, W = L->w, Cc = L->cout, N = m->N;
    if (n != (size_t)N * H * W * Cc) return fail(m, FCN8S_ERR_SHAPE, std::string("ReLU record of '") + layer + "' has " + std::to_string((size_t)N * H * W * Cc) + " elements");
    // layout of wino_output_kernel / wino_input_kernel / wino_out_in_kernel: RW words per (tile, channel vector), bit (oy * M + ox) * VEC + lane-channel
    const int tile = L->tile, vec = tile == 2 ? 4 : 2, RW = (tile * tile * vec + 31) / 32, C4 = Cc / vec;
    const int th = (H + tile - 1) / tile, tw = (W + tile - 1) / tile;
    const size_t words = wino_rbits_words(tile, N, H, W, Cc);
    std::vector<unsigned> w(words);
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(w.data(), L->rb, words * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int nn = 0; nn < N; ++nn)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t t = ((size_t)nn * th + y / tile) * tw + x / tile;
                const int oy = y % tile, ox = x % tile;
                unsigned char* dst = host + (((size_t)nn * H + y) * W + x) * Cc;
                for (int c = 0; c < Cc; ++c) {
                    const int bit = (oy * tile + ox) * vec + c % vec;
                    dst[c] = (w[(t * C4 + c / vec) * RW + (bit >> 5)] >> (bit & 31)) & 1u;
                }
            }
    return FCN8S_OK;
}

int fcn8s_get_pool_routing(fcn8s_model* m, int block, unsigned char* host, size_t n)
{
    if (!m || !host || block < 1 || block > 5) return FCN8S_ERR_BAD_ARG;
    if (!m->have_forward || !m->train_mode) return fail(m, FCN8S_ERR_STATE, "fcn8s_get_pool_routing: no training forward pass has been run");
    const Layer* last = nullptr;
    for (const Layer& L : m->layers) if (L.block == block && L.last_of_block()) last = &L;
    const int h = last->h, w = last->w, cw = last->cout;
    const size_t want = (size_t)m->N * (h / 2) * (w / 2) * cw;
    if (n != want) return fail(m, FCN8S_ERR_SHAPE, "pool routing of block " + std::to_string(block) + " has " + std::to_string(want) + " bytes");
    unsigned char* d = last->pidx;
    if (!pool_backward_fused(*last, m->pass.pool_fused[block - 1]) && !m->pass.pool_routed[block - 1]) {      // (pool_routed: the forward pool of bf16_train kept the bytes)
        // the backward pass routes through maxpool_bwd_kernel on the block's last conv output (materialised in this case): same rule
        launch_maxpool_route(last->y, d, m->N, h, w, cw, m->stream);
    }
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(host, d, n, hipMemcpyDeviceToHost));
    return FCN8S_OK;
}

int fcn8s_get_dropout_masks(fcn8s_model* m, float* h6, size_t n6, float* h7, size_t n7)
{
    if (!m || !m->have_forward) return fail(m, FCN8S_ERR_STATE, "no forward pass has been run");
    const Act& a6 = m->acts.at("fc6"); const Act& a7 = m->acts.at("fc7");
    if (n6 != a6.n || n7 != a7.n) return fail(m, FCN8S_ERR_SHAPE, "mask size mismatch");
    const float keep = ((m->train_mode || m->mc_masks) ? m->keep_prob : 1.f);
    DeviceBuf<float> d;
    if (!d.grow(std::max(n6, n7) * sizeof(float), m->stream)) return fail(m, FCN8S_ERR_OOM, "fcn8s_get_dropout_masks: out of device memory");
    launch_dropout_mask(d, (long long)n6, keep, m->seed, m->drop_stream, m->stream);
    hipMemcpyAsync(h6, d, n6 * sizeof(float), hipMemcpyDeviceToHost, m->stream);
    hipStreamSynchronize(m->stream);
    launch_dropout_mask(d, (long long)n7, keep, m->seed, m->drop_stream + 1, m->stream);
    hipMemcpyAsync(h7, d, n7 * sizeof(float), hipMemcpyDeviceToHost, m->stream);
    hipStreamSynchronize(m->stream);
    return FCN8S_OK;
}

int fcn8s_profile_enable(fcn8s_model* m, int on) { if (!m) return FCN8S_ERR_BAD_ARG; m->profile = on != 0; m->profile_detail = on == 2; return FCN8S_OK; }
int fcn8s_profile_reset(fcn8s_model* m)
{
    if (!m) return FCN8S_ERR_BAD_ARG;
    hipStreamSynchronize(m->stream);
    for (auto& g : m->groups) { for (auto& ev : g.ev) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); } g.ev.clear(); g.ev_shared.clear(); g.flops = g.bytes = 0; g.launches = 0; }
    return FCN8S_OK;
}
int fcn8s_profile_num_groups(const fcn8s_model* m) { return m ? (int)m->groups.size() : 0; }
int fcn8s_profile_get(fcn8s_model* m, int gi, const char** name, double* total_ms, int64_t* launches, double* flops, double* bytes)
{
    if (!m || gi < 0 || gi >= (int)m->groups.size()) return FCN8S_ERR_BAD_ARG;
    ProfGroup& g = m->groups[gi];
    HIPCHK(m, hipStreamSynchronize(m->stream));
    double ms = 0;
    for (auto& ev : g.ev) { float t = 0; if (hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) ms += t; }
    for (auto& ev : g.ev_shared) { float t = 0; if (hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) ms += t; }
    if (name) *name = g.name.c_str();
    if (total_ms) *total_ms = ms;
    if (launches) *launches = g.launches;
    if (flops) *flops = g.flops;
    if (bytes) *bytes = g.bytes;
    return FCN8S_OK;
}

// ---- single ops ------------------------------------------------------------------------------
#define OPCHK() do { { std::string t_; const int c_ = take_deferred_error(&t_); if (c_) return fail(nullptr, c_, t_); } \
                     hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(nullptr, FCN8S_ERR_HIP, hipGetErrorString(e_)); } while (0)

uint32_t fcn8s_crc32c(const void* data, size_t n, uint32_t crc)
{
    static uint32_t table[8][256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            table[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) table[t][i] = (table[t - 1][i] >> 8) ^ table[0][table[t - 1][i] & 0xFF];
        init = true;
    }
    const uint8_t* p = (const uint8_t*)data;
    uint32_t c = crc ^ 0xFFFFFFFFu;
    while (n >= 8) {                                   // slice-by-8
        uint32_t lo, hi; memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = table[7][lo & 0xFF] ^ table[6][(lo >> 8) & 0xFF] ^ table[5][(lo >> 16) & 0xFF] ^ table[4][lo >> 24] ^
            table[3][hi & 0xFF] ^ table[2][(hi >> 8) & 0xFF] ^ table[1][(hi >> 16) & 0xFF] ^ table[0][hi >> 24];
        p += 8; n -= 8;
    }
    while (n--) c = table[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

int fcn8s_onehot_to_ids(void* stream, const void* onehot, int elem_bytes, int64_t npix, int C, uint8_t* ids, int32_t* bad)
{
    if (!onehot || !ids || (elem_bytes != 1 && elem_bytes != 4) || C <= 0 || C > 255) return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_onehot_to_ids: bad argument");
    launch_onehot_to_ids(onehot, elem_bytes, npix, C, ids, bad, (hipStream_t)stream); OPCHK(); return FCN8S_OK;
}

int fcn8s_op_preprocess(void* stream, const void* images, int dtype, float* out4, int64_t npix)
{ launch_preprocess(images, dtype, out4, npix, (hipStream_t)stream); OPCHK(); return FCN8S_OK; }

int fcn8s_op_tta_input(void* stream, const uint8_t* images, int N, int H, int W, int Hs, int Ws, int Hp, int Wp, int flip, float* out4)
{
    if (!images || !out4 || N <= 0 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || Hp < Hs || Wp < Ws)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "tta_input: bad argument");
    launch_tta_input(images, FCN8S_IMG_U8, N, H, W, Hs, Ws, Hp, Wp, flip ? 1 : 0, out4, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_tta_accumulate(void* stream, const float* logits, int N, int Hp, int Wp, int Hs, int Ws, int flip, int C, int H, int W, float* acc,
                            int first, int last, int npasses, float* softmax_out, int64_t* argmax_out)
{
    if (!logits || N <= 0 || Hs <= 0 || Ws <= 0 || Hp < Hs || Wp < Ws || C <= 0 || H <= 0 || W <= 0 || npasses < 1 || (!acc && !(first && last))
        || (last && !softmax_out && !argmax_out) || ((uintptr_t)logits | (uintptr_t)acc | (uintptr_t)softmax_out) % 16)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "tta_accumulate: bad argument");
    const PixMap pm{0, Hp, Wp, 0, 0, 0};
    launch_tta_accumulate(logits, pm, N, Hs, Ws, flip ? 1 : 0, C, H, W, acc, first ? 1 : 0, last ? 1 : 0, npasses, softmax_out, (long long*)argmax_out, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_mc_accumulate(void* stream, const float* logits, int N, int H, int W, int C, float* acc, float* ent_acc, int first, int last, int nsamples,
                           float* softmax_out, int64_t* argmax_out, float* entropy_out, float* mi_out)
{
    if (!logits || N <= 0 || H <= 0 || W <= 0 || C <= 0 || nsamples < 1 || ((!acc || !ent_acc) && !(first && last))
        || ((uintptr_t)logits | (uintptr_t)acc | (uintptr_t)softmax_out) % 16)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "mc_accumulate: bad argument");
    const PixMap pm{0, H, W, 0, 0, 0};
    launch_mc_accumulate(logits, pm, N, H, W, C, acc, ent_acc, first ? 1 : 0, last ? 1 : 0, nsamples, softmax_out, (long long*)argmax_out, entropy_out, mi_out, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}

size_t fcn8s_op_crf_work_floats(int N, int H, int W, int C, const fcn8s_crf_params* p)
{
    if (!p || N <= 0 || H <= 0 || W <= 0 || C <= 0 || crf_bad_field(p) || p->iterations == 0) return 0;
    return 2 * (size_t)N * H * W * C;
}
int fcn8s_op_crf_meanfield(void* stream, const float* prob, const uint8_t* images, int N, int H, int W, int C, const fcn8s_crf_params* p,
                           float* work, float* q_out, int64_t* argmax_out)
{
    if (!p) return fail(nullptr, FCN8S_ERR_BAD_ARG, "crf_meanfield: null crf_params");
    if (const char* bad = crf_bad_field(p)) return fail(nullptr, FCN8S_ERR_BAD_ARG, std::string("crf_meanfield: crf_params.") + bad + " is out of range");
    if (!prob || !images || (!q_out && !argmax_out) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || prob == q_out || (p->iterations > 0 && !work)
        || ((uintptr_t)prob | (uintptr_t)work | (uintptr_t)q_out) % 16)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "crf_meanfield: bad argument (null or unaligned pointer, C not a multiple of 4, q_out == prob)");
    if (!crf_shape_supported(C, p->radius)) return fail(nullptr, FCN8S_ERR_SHAPE, "crf_meanfield: this many classes do not fit the LDS tile at this radius");
    hipStream_t s = (hipStream_t)stream;
    take_deferred_error(nullptr);
    if (p->iterations == 0) {
        if (q_out && hipMemcpyAsync(q_out, prob, (size_t)N * H * W * C * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(nullptr, FCN8S_ERR_HIP, "crf_meanfield: the copy of prob failed");
        if (argmax_out) launch_crf_argmax(prob, (long long)N * H * W, C, (long long*)argmax_out, s);
    } else {
        crf_run(nullptr, s, prob, images, N, H, W, C, p, work, q_out, (long long*)argmax_out);
    }
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_augment_u8(void* stream, const uint8_t* images, const uint8_t* labels, uint8_t* out_images, uint8_t* out_labels,
                        const int32_t* params, const uint8_t* vlut, int N, int H, int W, int Ho, int Wo, int void_id)
{
    if (!images || !out_images || !params || N <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || (labels && !out_labels))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "augment_u8: bad argument");
    launch_augment_u8(images, labels, out_images, out_labels, params, vlut, N, H, W, Ho, Wo, void_id, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_resample_u8(void* stream, const uint8_t* images, const uint8_t* labels, uint8_t* out_images, uint8_t* out_labels,
                         const int32_t* params, int N, int H, int W, int Ho, int Wo, int void_id)
{
    if ((!images && !labels) || (images && !out_images) || (labels && !out_labels) || !params || N <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "resample_u8: bad argument");
    launch_resample_u8(images, labels, images ? out_images : nullptr, labels ? out_labels : nullptr, params, N, H, W, Ho, Wo, void_id, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_conv2d(void* stream, const float* x, const float* w, const float* bias, float* y,
                    int N, int H, int W, int Cin, int Cout, int K, int relu)
{
    if (Cin % 4 || Cout % 4 || K % 2 == 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d: Cin, Cout must be multiples of 4 and K odd");
    FwdEpi e; e.bias = bias; e.relu = relu;
    if (K == 1 && Cout <= 32 && !relu && N > 0 && H > 0 && W > 0) {
        // a score head: a bare model whose idle filter-bank scratch is large enough for the eight-slab form, as a model's is -- whether
        // the launch splits is then launch_head_fwd's decision (split_route.h), as in a model, and not a matter of a missing scratch
        hipStream_t s = (hipStream_t)stream;
        fcn8s_model mm; fcn8s_model* m = &mm;
        m->stream = s; m->N = N; m->H = H; m->W = W;
        m->precision = t_op_split == 3 ? FCN8S_PREC_F32X3 : t_op_split == 2 ? FCN8S_PREC_F32X2 : FCN8S_PREC_F32;
        m->ufl = (size_t)8 * N * H * W * Cout;
        if (!m->d_wino_u.grow(m->ufl * sizeof(float), s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
        hipMemsetAsync(m->d_wino_u, 0xFF, m->ufl * sizeof(float), s);          // NaN: in a model these slabs hold the last filter bank
        conv_fwd(m, "", x, w, y, N, H, W, Cin, Cout, K, e, s);
        hipStreamSynchronize(s);
        OPCHK(); return FCN8S_OK;
    }
    conv_fwd(nullptr, "", x, w, y, N, H, W, Cin, Cout, K, e, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_conv2d_winograd(void* stream, const float* x, const float* w, const float* bias, float* y,
                             int N, int H, int W, int Cin, int Cout, int K, int relu, int tile)
{
    if ((tile != 2 && tile != 4 && tile != 6) || (K != 3 && K != 7) || (K == 7 && tile != 4) || Cin % 16 || Cout % 32 || (tile != 6 && (H % tile || W % tile)) || H % 2 || W % 2)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_winograd: needs tile in {2,4,6} (4 for K = 7), K in {3,7}, Cin % 16, Cout % 32, even H and W (multiples of tile for tile 2 and 4)");
    hipStream_t s = (hipStream_t)stream;
    const size_t T = (size_t)wino_tiles(tile, N, H, W), P = (size_t)wino_alpha(tile, K) * wino_alpha(tile, K), Kg = (size_t)wino_nsub(K) * wino_nsub(K) * Cin;
    DeviceBuf<float> u, v, mm;
    if (!u.grow(P * Kg * Cout * 4, s) || !v.grow(P * (size_t)wino_slab(T, (int)Kg) * 4, s) || !mm.grow(P * (size_t)wino_slab(T, Cout) * 4, s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
    // all of it NaN, as in fcn8s_op_conv3x3_winograd_pool: what a model's workspace holds behind a slab or beyond row T is another layer's leftovers
    hipMemsetAsync(u, 0xFF, u.bytes(), s); hipMemsetAsync(v, 0xFF, v.bytes(), s); hipMemsetAsync(mm, 0xFF, mm.bytes(), s);
    WinoEpi we; we.bias = bias; we.relu = relu;
    conv_winograd(nullptr, tile, K, true, x, w, y, u, v, mm, N, H, W, Cin, Cout, we, s, nullptr);
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_conv3x3_winograd_fwd_bwd(void* stream, const float* x, const float* w, const float* bias, const float* dy, const float* dx_addend,
                                      float* y, float* pool, float* dx, float* dw, float* db,
                                      int N, int H, int W, int Cin, int Cout, int tile, int pooled, int mask_mode)
{
    if ((tile != 2 && tile != 4 && tile != 6) || Cin % 64 || Cout % 64 || H % 2 || W % 2 || (tile != 6 && (H % tile || W % tile)) || !x || !w || !dy || !dx || !dw ||
        (pooled && (!pool || tile < 4)) || (!pooled && !y) || mask_mode < 0 || mask_mode > 2)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv3x3_winograd_fwd_bwd: needs tile in {2,4,6}, Cin % 64 == 0, Cout % 64 == 0, even H and W (multiples of tile for tiles 2, 4), "
                                                "pooled only with tiles 4 and 6, mask_mode in {0,1,2}");
    hipStream_t s = (hipStream_t)stream;
    // a bare model context: the launch sequences below are the model's own (conv_fwd / conv_wgrad / conv_dgrad), with one layer called "op"
    fcn8s_model mm; fcn8s_model* m = &mm;
    m->stream = s; m->wino_min_cin = 16; m->wino_tile = 6; m->wino_force_tile = tile; m->N = N; m->H = H; m->W = W;
    m->precision = t_op_split == 3 ? FCN8S_PREC_F32X3 : t_op_split == 2 ? FCN8S_PREC_F32X2 : FCN8S_PREC_F32;
    const int al = tile + 2, P = al * al, cmax = std::max(Cin, Cout);
    const size_t T = (size_t)wino_tiles(tile, N, H, W);
    const size_t slab_max = (size_t)P * (size_t)wino_slab((long long)T, cmax), slab_in = (size_t)P * (size_t)wino_slab((long long)T, Cin);
    // (what the model keeps in its arena is this call's own; the model frees d_wino_u and the banks it makes behind this function's back)
    DeviceBuf<float> wino_v, wino_m, wv, wt, pidx, rbits;
    bool ok = true;
    auto dalloc = [&](DeviceBuf<float>& b, size_t nfloats) {          // all of it NaN, as in fcn8s_op_conv3x3_winograd_pool
        ok = ok && b.grow(nfloats * sizeof(float), s);
        if (ok) hipMemsetAsync(b, 0xFF, nfloats * sizeof(float), s);
    };
    m->ufl = (size_t)P * cmax * cmax + (t_op_fused64 ? wino_gemm_out64_bank_floats() : 0);       // (the second, MFMA-ordered bank behind the first)
    if (t_op_fused64 == 2) m->gemm_out64_nt = 1;
    dalloc(m->d_wino_u, m->ufl); dalloc(wino_v, slab_max); dalloc(wino_m, slab_max);
    dalloc(wv, slab_in); dalloc(wt, (size_t)9 * Cin * Cout);
    if (pooled) dalloc(pidx, ((size_t)N * (H / 2) * (W / 2) * Cout + 3) / 4);
    if (mask_mode == 2) dalloc(rbits, wino_rbits_words(tile, N, H, W, Cin));
    if (!ok) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
    m->d_wino_v = wino_v; m->d_wino_m = wino_m;
    Act a; a.p = wv; a.n = slab_in; m->acts["wv:op"] = a;
    // forward (training mode: keeps V and the filter bank, writes the pool argmax bytes / the input's ReLU bit record)
    m->fwd_train = true; m->train_mode = true;
    { FwdEpi e; e.bias = bias; e.relu = 1;
      e.gemm_out_fused64 = t_op_fused64 != 0;            // asked for: whether the kernel runs is conv_winograd's decision
      if (pooled) { e.pool_out = pool; e.pool_idx = (unsigned char*)pidx.get(); e.skip_y = y == nullptr; }
      if (mask_mode == 2) { e.in_relu_bits_out = (unsigned*)rbits.get(); e.in_layer = "prev"; }
      conv_fwd(m, "op", x, w, y, N, H, W, Cin, Cout, 3, e, s, 0, "op"); }
    // backward: weight + bias gradient in the Winograd domain, then the data gradient (adjoint form for tile 6)
    hipMemsetAsync(dw, 0, (size_t)9 * Cin * Cout * sizeof(float), s);
    if (db) hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s);
    conv_wgrad(m, "op", x, dy, dw, db, N, H, W, Cin, Cout, 3, 1.f, s, 0, "op", pooled ? (const unsigned char*)pidx.get() : nullptr);
    { DgradEpi e; e.w_fwd = w; e.lazy_wt = 1; e.addend = dx_addend;
      if (mask_mode) { e.mask = x; e.mask_scale = 1.f; }
      if (mask_mode == 2 && m->pass.rbits_ok.count("prev")) e.relu_bits_in = (const unsigned*)rbits.get();
      conv_dgrad(m, "op", dy, wt, dx, N, H, W, Cout, Cin, 3, e, s, "op"); }
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}

// One 3x3 SAME conv + bias + ReLU + 2x2/2 max-pool the way the last conv of a block runs forward: the model's own conv_fwd on a bare model with
// one layer called "op", the full-resolution output never written.  train: V is kept in the layer's own slot, the bank in u_train, the argmax
// bytes go to pidx; else (as fcn8s_predict) V goes to the shared scratch and no bytes are written.  Whether wino_gemm_out64_kernel runs (op context
// "op_gemm_out_fused64") is conv_winograd's decision; *fused reports it.  Every scratch buffer is an allocation of its own, all of it NaN: what a
// model's shared workspace holds behind a slab is another layer's leftovers.  For tests only: it allocates and synchronises per call.
int fcn8s_op_conv3x3_winograd_pool(void* stream, const float* x, const float* w, const float* bias, float* pool, unsigned char* pidx,
                                   int N, int H, int W, int Cin, int Cout, int tile, int train, int* fused)
{
    if (fused) *fused = 0;
    if ((tile != 4 && tile != 6) || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 64 || Cout % 64 || H % 2 || W % 2 || (tile != 6 && (H % tile || W % tile)) ||
        !x || !w || !bias || !pool)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv3x3_winograd_pool: needs tile in {4,6}, Cin % 64 == 0, Cout % 64 == 0, even H and W (multiples of 4 for tile 4), non-null x, w, bias, pool");
    hipStream_t s = (hipStream_t)stream;
    fcn8s_model mm; fcn8s_model* m = &mm;
    m->stream = s; m->wino_min_cin = 16; m->wino_tile = 6; m->wino_force_tile = tile; m->N = N; m->H = H; m->W = W;
    m->precision = t_op_split == 3 ? FCN8S_PREC_F32X3 : t_op_split == 2 ? FCN8S_PREC_F32X2 : FCN8S_PREC_F32;
    if (t_op_fused64 == 2) m->gemm_out64_nt = 1;
    const int al = tile + 2, P = al * al, cmax = std::max(Cin, Cout);
    const long long T = wino_tiles(tile, N, H, W);
    const size_t v_floats = (size_t)P * (size_t)wino_slab(T, Cin), m_floats = (size_t)P * (size_t)wino_slab(T, Cout);
    DeviceBuf<float> wino_v, wino_m, wv;
    bool ok = true;
    auto dalloc = [&](DeviceBuf<float>& b, size_t nfloats) {
        ok = ok && b.grow(nfloats * sizeof(float), s);
        if (ok) hipMemsetAsync(b, 0xFF, nfloats * sizeof(float), s);
    };
    // (the bank with room for the second, MFMA-ordered copy behind it: the inference call has no u_train to put them in)
    m->ufl = (size_t)P * cmax * cmax + wino_gemm_out64_bank_floats();
    dalloc(m->d_wino_u, m->ufl); dalloc(wino_v, v_floats); dalloc(wino_m, m_floats);
    if (train) dalloc(wv, v_floats);
    if (!ok) { hipStreamSynchronize(s); return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc"); }
    m->d_wino_v = wino_v; m->d_wino_m = wino_m;
    if (train) { Act a; a.p = wv; a.n = v_floats; m->acts["wv:op"] = a; }
    m->fwd_train = train != 0; m->train_mode = train != 0;
    { FwdEpi e; e.bias = bias; e.relu = 1; e.pool_out = pool; e.skip_y = 1;
      if (train) e.pool_idx = pidx;
      e.gemm_out_fused64 = t_op_fused64 != 0;
      conv_fwd(m, "op", x, w, nullptr, N, H, W, Cin, Cout, 3, e, s, 0, "op"); }
    if (fused) *fused = m->gemm_out64_launches > 0;
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}

// One 7x7 SAME convolution the way fc6 runs in an fp32 training step: conv_fwd in training mode, conv_wgrad, conv_dgrad, on a bare
// model with one layer called "op" -- which of the DFT tiles, F(4x4,4x4) and the direct kernels run is decided by the model's own rules (fft6_on,
// fft6_wgrad_wanted, bt_gemm_ok, wino_tile_for), never by this function.  For tests only: it allocates and synchronises per call, so it says nothing about time.
int fcn8s_op_conv7x7_fc6_fwd_bwd(void* stream, const float* x, const float* w, const float* bias, const float* dy,
                                 float* y, float* dx, float* dw, float* db,
                                 int N, int H, int W, int Cin, int Cout, int path, float keep_prob, uint64_t seed, int* dft_products)
{
    if (dft_products) *dft_products = 0;
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 16 || Cout % 128 || path < 0 || path > 2 || !(keep_prob > 0.f && keep_prob <= 1.f) ||
        !x || !w || !dy || !y || !dx || !dw)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv7x7_fc6_fwd_bwd: needs Cin % 16 == 0, Cout % 128 == 0, path in {0,1,2}, keep_prob in (0, 1], non-null x, w, dy, y, dx, dw");
    hipStream_t s = (hipStream_t)stream;
    fcn8s_model mm; fcn8s_model* m = &mm;
    m->stream = s; m->N = N; m->H = H; m->W = W; m->plan_N = N; m->seed = seed; m->keep_prob = keep_prob;
    m->precision = t_op_split == 3 ? FCN8S_PREC_F32X3 : t_op_split == 2 ? FCN8S_PREC_F32X2 : FCN8S_PREC_F32;
    m->fc6_fft = path != 0; m->fc6_fft_wgrad = path == 2 ? 2 : 0;
    m->profile = true;                     // the launch counts of the three DFT plane GEMMs are what dft_products reports
    // the scratch exactly as the model plans it for this shape (plan_workspace, fcn8s_create), each buffer an allocation of its own, all of it NaN:
    // what a model's shared workspace holds behind a slab or a partial row tile is another layer's leftovers
    const Fc6Scratch f6 = fc6_scratch_floats(m, N, H, W, Cin, Cout);
    const size_t vmax = std::max(f6.v_wino, f6.v_fft), mmax = std::max(f6.v_wino, f6.m_fft);
    DeviceBuf<float> wino_v, wino_m, wv, wt;               // (wt: the flipped + transposed kernel of a forward-type data gradient, the model's d_wt)
    bool ok = true;
    auto dalloc = [&](DeviceBuf<float>& b, size_t nfloats, bool poison, const char* slot = nullptr) {      // slot: also one of the model's named arena items
        ok = ok && b.grow(nfloats * sizeof(float), s);
        if (ok && poison) hipMemsetAsync(b, 0xFF, nfloats * sizeof(float), s);
        if (ok && slot) { Act a; a.p = b; a.n = nfloats; m->acts[slot] = a; }
    };
    if (vmax) { dalloc(wino_v, vmax, true, "wino_v"); dalloc(wino_m, mmax, true, "wino_m"); m->d_wino_v = wino_v; m->d_wino_m = wino_m; }
    if (f6.wv) dalloc(wv, f6.wv, true, "wv:op");
    m->ufl = fc6_bank_floats(Cin, Cout);
    dalloc(m->d_wino_u, m->ufl, true);
    dalloc(wt, (size_t)49 * Cin * Cout, false);
    if (!ok) { hipStreamSynchronize(s); return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc"); }
    // forward, as forward() runs fc6 (step 0: dropout stream 0)
    m->fwd_train = true; m->train_mode = true; m->drop_stream = 0;
    { FwdEpi e; e.bias = bias; e.relu = 1; e.dropout = keep_prob < 1.f; e.keep = keep_prob; e.stream_id = m->drop_stream;
      conv_fwd(m, "fc6_fwd", x, w, y, N, H, W, Cin, Cout, 7, e, s, 0, "op"); }
    // backward, as backward_fc6 runs it: the weight gradient first (it may leave dYf / dM for the data gradient), then the data gradient
    hipMemsetAsync(dw, 0, (size_t)49 * Cin * Cout * sizeof(float), s);
    if (db) hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s);
    conv_wgrad(m, "fc6_wgrad", x, dy, dw, db, N, H, W, Cin, Cout, 7, 1.f, s, 0, "op");
    { DgradEpi e; e.w_fwd = w; e.lazy_wt = 1;
      conv_dgrad(m, "fc6_dgrad", dy, wt, dx, N, H, W, Cout, Cin, 7, e, s, "op"); }
    if (dft_products)
        for (const auto& g : m->groups) {
            if (g.launches <= 0) continue;
            if (g.name == "fc6_fft_gemm_fwd") *dft_products |= 1;
            if (g.name == "fc6_fft_gemm_wgrad") *dft_products |= 2;
            if (g.name == "fc6_fft_gemm_dgrad") *dft_products |= 4;
        }
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_conv2d_bf16(void* stream, const float* x, const float* w, const float* bias, float* y,
                         int N, int H, int W, int Cin, int Cout, int K, int relu)
{
    if (Cin % 32 || Cout % 128 || K % 2 == 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_bf16: needs Cin % 32 == 0, Cout % 128 == 0, K odd");
    hipStream_t s = (hipStream_t)stream;
    DeviceBuf<unsigned short> wt;
    if (!wt.grow((size_t)K * K * Cin * Cout * 2, s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
    hipMemsetAsync(wt, 0xFF, wt.bytes(), s);          // (bf16 NaNs)
    launch_w_to_bf16_tiles(w, wt, K * K * Cin, Cout, s);
    Bf16ConvArgs a{};
    a.x = x; a.wt = wt; a.bias = bias; a.y = y; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.K = K; a.relu = relu;
    launch_conv_bf16(a, s);
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}

// One K x K SAME convolution in the arithmetic of FCN8S_PREC_BF16_TRAIN on the kernels that mode runs (gemm_bf16.hip): any of y (forward, + bias,
// optional ReLU), dx (data gradient of dy, optional mask: dx = mask > 0 ? dx : 0), dw / db (weight / bias gradient) may be NULL.
int fcn8s_op_conv2d_bf16_train(void* stream, const float* x, const float* w, const float* bias, float* y, int relu,
                               const float* dy, const float* mask, float* dx, float* dw, float* db,
                               int N, int H, int W, int Cin, int Cout, int K)
{
    if (Cin % 64 || Cout % 64 || K % 2 == 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_bf16_train: needs Cin % 64 == 0, Cout % 64 == 0, K odd");
    hipStream_t s = (hipStream_t)stream;
    const int pad = (K - 1) / 2, Wp_ = W + 2 * pad;
    const long long G = bf16_guard_rows(K, Wp_), R = (long long)N * (H + 2 * pad) * Wp_;
    // the padded copies as channel-chunk planes [C / 32][G + R + G][32], as the bf16_train mode keeps them (op option "op_bf16_planes" = 0: [rows][C], the
    // layout every kernel still takes -- plane stride 0 -- and the other bf16 modes use)
    const long long PS = t_op_planes ? (R + 2 * G) * 32 : 0;
    const long long OX = t_op_planes ? G * 32 : G * Cin, OY = t_op_planes ? G * 32 : G * Cout;
    DeviceBuf<unsigned short> xb, dyb, wt;
    const size_t nx = (size_t)(R + 2 * G) * Cin, ny = (size_t)(R + 2 * G) * Cout, nw = (size_t)K * K * Cin * Cout;
    if (!wt.grow(nw * 2, s) || (x && !xb.grow(nx * 2, s, nullptr, true)) || (dy && !dyb.grow(ny * 2, s, nullptr, true))) { hipStreamSynchronize(s); return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc"); }
    // (bf16 NaNs in the weight copy; xb and dyb stay zeroed: their zero border and guard rows ARE the padding, interleaved with the interior row by row)
    hipMemsetAsync(wt, 0xFF, wt.bytes(), s);
    if (x) {
        launch_f32_to_bf16_padded(x, xb + OX, N, H, W, Cin, pad, s, PS);
    }
    if (dy) {
        launch_f32_to_bf16_padded(dy, dyb + OY, N, H, W, Cout, pad, s, PS);
    }
    bool ok = true;
    if (y && x && w) {
        launch_w_to_bf16_t(w, wt, K * K * Cin, Cout, s);
        Bf16Conv256Args g{};
        g.xp = xb + OX; g.xp_ps = PS; g.wt = wt; g.bias = bias; g.y = y; g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.K = K; g.relu = relu; g.any_shape = 1; g.mask_scale = 1.f; g.guarded = 1; g.rows_bn = t_op_rows_bn;
        ok = ok && launch_conv_bf16_256(g, s);
    }
    if (dx && dy && w) {
        launch_w_to_bf16_flip_t(w, wt, K, Cin, Cout, s);
        Bf16Conv256Args g{};
        g.xp = dyb + OY; g.xp_ps = PS; g.wt = wt; g.y = dx; g.N = N; g.H = H; g.W = W; g.Cin = Cout; g.Cout = Cin; g.K = K; g.mask = mask; g.mask_scale = 1.f; g.any_shape = 1; g.guarded = 1; g.rows_bn = t_op_rows_bn;
        ok = ok && launch_conv_bf16_256(g, s);
    }
    if (dw && x && dy) {
        Bf16WgradArgs g{};
        g.A = xb + OX; g.B = dyb + OY; g.a_ps = g.b_ps = PS; g.C = dw; g.R = R; g.Ci = Cin; g.Cj = Cout; g.K = K; g.Wp = Wp_;
        ok = ok && launch_wgrad_bf16(g, s);
    }
    if (db && dy) { hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s); launch_colsum(dy, db, (long long)N * H * W, Cout, s); }
    hipStreamSynchronize(s);
    if (!ok) return fail(nullptr, FCN8S_ERR_SHAPE, "conv2d_bf16_train: a launch refused the shape");
    OPCHK(); return FCN8S_OK;
}

// One K x K SAME convolution in the arithmetic of FCN8S_PREC_FP8_INFER on that mode's kernels (gemm_fp8.hip): x quantized with exponent x_exp into a padded
// e4m3 copy, w per output channel, y = 2^(x_exp + ew) sum Xq Wq + bias (ReLU if relu)
int fcn8s_op_conv2d_fp8(void* stream, const float* x, const float* w, const float* bias, float* y, int relu, int x_exp,
                        int N, int H, int W, int Cin, int Cout, int K)
{
    if (!x || !w || !y) return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_fp8: null argument");
    if (Cin % 64 || Cout % 64 || K % 2 == 0 || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_fp8: needs Cin % 64 == 0, Cout % 64 == 0, K odd, positive sizes");
    hipStream_t s = (hipStream_t)stream;
    const int pad = (K - 1) / 2;
    const long long R = (long long)N * (H + 2 * pad) * (W + 2 * pad);
    const size_t xb = (size_t)R * Cin, wb = (size_t)K * K * Cin * Cout;
    DeviceBuf<unsigned char> xq, wq;
    if (!xq.grow(xb, s, nullptr, true) || !wq.grow(wb + 8 * (size_t)Cout, s)) { hipStreamSynchronize(s); return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc"); }
    hipMemsetAsync(wq, 0xFF, wq.bytes(), s);          // (e4m3 NaNs, exponents of -1; xq stays zeroed: its zero border is the padding)
    launch_f32_to_fp8_padded(x, xq, N, H, W, Cin, pad, R * 64, x_exp, s);
    int* ew = reinterpret_cast<int*>(wq + wb);
    launch_w_to_fp8(w, wq, ew, reinterpret_cast<unsigned*>(wq + wb + 4 * (size_t)Cout), K * K * Cin, Cout, s);
    Fp8ConvArgs a;
    a.xp = xq; a.xp_ps = R * 64; a.wq = wq; a.ew = ew; a.bias = bias; a.y = y; a.ex = x_exp; a.relu = relu;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.K = K; a.M = (long long)N * H * W;
    const bool ok = launch_conv_fp8(a, s);
    hipStreamSynchronize(s);
    if (!ok) return fail(nullptr, FCN8S_ERR_SHAPE, "conv2d_fp8: the launch refused the shape");
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_conv2d_bwd(void* stream, const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                        int N, int H, int W, int Cin, int Cout, int K)
{
    if (Cin % 4 || Cout % 4 || K % 2 == 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_bwd: Cin, Cout must be multiples of 4 and K odd");
    hipStream_t s = (hipStream_t)stream;
    if (dw) {
        hipMemsetAsync(dw, 0, (size_t)K * K * Cin * Cout * sizeof(float), s);
        if (db) hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s);
        conv_wgrad(nullptr, "", x, dy, dw, db, N, H, W, Cin, Cout, K, 1.f, s);
    } else if (db) { hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s); launch_colsum(dy, db, (long long)N * H * W, Cout, s); }
    if (dx) {
        DeviceBuf<float> wt;
        if (!wt.grow((size_t)K * K * Cin * Cout * sizeof(float), s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
        hipMemsetAsync(wt, 0xFF, wt.bytes(), s);
        launch_flip_transpose(w, wt, K * K, Cin, Cout, s);
        conv_dgrad(nullptr, "", dy, wt, dx, N, H, W, Cout, Cin, K, DgradEpi{}, s);
        hipStreamSynchronize(s);
    }
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_maxpool2x2(void* stream, const float* x, float* y, int N, int H, int W, int C)
{
    if (C % 4 || H % 2 || W % 2) return fail(nullptr, FCN8S_ERR_BAD_ARG, "maxpool: C%4, H%2, W%2 must be 0");
    launch_maxpool_fwd(x, y, N, H, W, C, (hipStream_t)stream); OPCHK(); return FCN8S_OK;
}
int fcn8s_op_maxpool2x2_bwd(void* stream, const float* x, const float* dy, float* dx, int N, int H, int W, int C, int relu_mask)
{
    if (C % 4 || H % 2 || W % 2) return fail(nullptr, FCN8S_ERR_BAD_ARG, "maxpool: C%4, H%2, W%2 must be 0");
    launch_maxpool_bwd(x, dy, dx, N, H, W, C, relu_mask, (hipStream_t)stream); OPCHK(); return FCN8S_OK;
}

int fcn8s_op_conv2d_transpose(void* stream, const float* x, const float* w, const float* bias, const float* addend, float* y,
                              int N, int Hi, int Wi, int C, int K, int S)
{
    if (C % 4 || K != 2 * S) return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_transpose: needs C%4==0 and K == 2*S");
    hipStream_t s = (hipStream_t)stream;
    DeviceBuf<float> wp;
    if (!wp.grow((size_t)S * S * 4 * C * C * sizeof(float), s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
    hipMemsetAsync(wp, 0xFF, wp.bytes(), s);
    launch_tconv_phase_pack(w, wp, K, S, C, s);
    tconv_fwd(nullptr, x, wp, bias, addend, y, N, Hi, Wi, C, K, S, s);
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_conv2d_transpose_bwd(void* stream, const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                                  int N, int Hi, int Wi, int C, int K, int S)
{
    if (C % 4 || K != 2 * S) return fail(nullptr, FCN8S_ERR_BAD_ARG, "conv2d_transpose_bwd: needs C%4==0 and K == 2*S");
    hipStream_t s = (hipStream_t)stream;
    if (dw) { hipMemsetAsync(dw, 0, (size_t)K * K * C * C * sizeof(float), s); tconv_wgrad(nullptr, x, dy, dw, N, Hi, Wi, C, K, S, s); }
    if (db) { hipMemsetAsync(db, 0, (size_t)C * sizeof(float), s); launch_colsum(dy, db, (long long)N * Hi * S * Wi * S, C, s); }
    if (dx) tconv_dgrad(nullptr, dy, w, dx, N, Hi, Wi, C, K, S, s);
    OPCHK(); return FCN8S_OK;
}

int fcn8s_op_softmax_xent(void* stream, const float* logits, const uint8_t* labels, float* dlogits, float* loss_dev, int64_t npix, int C)
{
    hipStream_t s = (hipStream_t)stream;
    DeviceBuf<double> part;
    if (!part.grow(4096 * sizeof(double), s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
    launch_softmax_xent(logits, labels, dlogits, part, npix, C, 1.0f / (float)npix, s);
    launch_finalize_loss(part, softmax_xent_blocks(npix), npix, nullptr, 0.f, loss_dev, s);
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}
// fcn8s_op_softmax_xent_ex / _px (`who`: the entry point's name for the error texts); codes_dev and table256_dev both set or both nullptr
static int op_softmax_xent_weighted(const char* who, void* stream, const float* logits, const uint8_t* labels, const float* class_weights_dev,
                                    float ohem_thresh, int64_t ohem_min_kept, const uint8_t* codes_dev, const float* table256_dev, float* dlogits,
                                    float* loss_dev, float* pixel_loss_dev, int64_t* stats_dev, int64_t npix, int C)
{
    if (!class_weights_dev && ohem_thresh == 0.f && !codes_dev) return fcn8s_op_softmax_xent(stream, logits, labels, dlogits, loss_dev, npix, C);
    if (!logits || !labels || !loss_dev || npix < 1 || C < 1 || C > 64) return fail(nullptr, FCN8S_ERR_BAD_ARG, std::string(who) + ": bad argument");
    int rc = check_loss_args(nullptr, nullptr, C, C, ohem_thresh, ohem_min_kept, who); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool ohem = ohem_thresh > 0.f;
    const size_t lb = ohem && !pixel_loss_dev ? (size_t)npix * sizeof(float) : 0;
    DeviceBuf<char> ws;
    if (!ws.grow(4096 * sizeof(double) + 64 * sizeof(float) + LOSS_SCRATCH_BYTES + lb, s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
    double* part = (double*)ws.get();
    float* ones = (float*)(ws + 4096 * sizeof(double));
    char* sc = ws + 4096 * sizeof(double) + 64 * sizeof(float);
    if (!class_weights_dev) { const std::vector<float> h(64, 1.f); hipMemcpyAsync(ones, h.data(), 64 * sizeof(float), hipMemcpyHostToDevice, s); hipStreamSynchronize(s); }
    XentEx x; x.cw = class_weights_dev ? class_weights_dev : ones; x.st = (OhemState*)sc; x.hist = (unsigned*)(sc + sizeof(OhemState));
    x.lbuf = ohem ? (pixel_loss_dev ? pixel_loss_dev : (float*)(sc + LOSS_SCRATCH_BYTES)) : nullptr;
    x.codes = codes_dev; x.ptab = table256_dev;
    launch_softmax_xent_ex(logits, labels, dlogits, part, npix, C, 1.0f / (float)npix, s, nullptr, nullptr, 0, x, ohem_thresh, (long long)ohem_min_kept);
    launch_finalize_loss(part, softmax_xent_blocks(npix), npix, nullptr, 0.f, loss_dev, s, ohem ? &x.st->kept : nullptr);
    OhemState st{};
    hipMemcpyAsync(&st, x.st, sizeof st, hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    if (stats_dev) {
        uint32_t tb = 0; const float t = ohem ? st.t : 0.f; std::memcpy(&tb, &t, 4);
        const int64_t h[3] = {(int64_t)st.valid, (int64_t)(ohem ? st.kept : st.valid), (int64_t)tb};
        hipMemcpy(stats_dev, h, sizeof h, hipMemcpyHostToDevice);
    }
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_softmax_xent_ex(void* stream, const float* logits, const uint8_t* labels, const float* class_weights_dev, float ohem_thresh,
                             int64_t ohem_min_kept, float* dlogits, float* loss_dev, float* pixel_loss_dev, int64_t* stats_dev, int64_t npix, int C)
{
    return op_softmax_xent_weighted("fcn8s_op_softmax_xent_ex", stream, logits, labels, class_weights_dev, ohem_thresh, ohem_min_kept, nullptr, nullptr,
                                    dlogits, loss_dev, pixel_loss_dev, stats_dev, npix, C);
}
int fcn8s_op_softmax_xent_px(void* stream, const float* logits, const uint8_t* labels, const float* class_weights_dev, float ohem_thresh,
                             int64_t ohem_min_kept, const uint8_t* codes_dev, const float* table256_dev, float* dlogits, float* loss_dev,
                             float* pixel_loss_dev, int64_t* stats_dev, int64_t npix, int C)
{
    if (!codes_dev != !table256_dev) return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_op_softmax_xent_px: codes and table must both be given or both be NULL");
    return op_softmax_xent_weighted("fcn8s_op_softmax_xent_px", stream, logits, labels, class_weights_dev, ohem_thresh, ohem_min_kept, codes_dev,
                                    table256_dev, dlogits, loss_dev, pixel_loss_dev, stats_dev, npix, C);
}
int fcn8s_op_lovasz_softmax(void* stream, const float* x, int x_is_logits, const uint8_t* labels, int64_t nseg, int64_t seg_pixels, int C,
                            int classes_all, const uint8_t* class_mask_dev, float* loss_out_dev, float* grad_out, float* class_loss_out)
{
    if (!x || !labels || !loss_out_dev || nseg < 1 || seg_pixels < 1 || C < 1 || C > 64 || (x_is_logits != 0 && x_is_logits != 1) ||
        (classes_all != 0 && classes_all != 1) || nseg > 65535 || seg_pixels >= (1LL << 31))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "fcn8s_op_lovasz_softmax: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)nseg * seg_pixels;
    const LovaszLayout y = lovasz_layout(npix, (int)nseg, C);
    DeviceBuf<char> ws;
    if (!ws.grow(y.bytes, s)) return fail(nullptr, FCN8S_ERR_OOM, "hipMalloc");
    launch_lovasz_loss(x, x_is_logits, labels, nullptr, 0, npix, y, classes_all, class_mask_dev, ws, class_loss_out, nullptr, 1.f, 1.f, nullptr, s);
    hipMemcpyAsync(loss_out_dev, ws + y.o_lov, sizeof(float), hipMemcpyDeviceToDevice, s);
    if (grad_out) launch_lovasz_backward(x, x_is_logits, labels, nullptr, 0, npix, y, ws, 1.f, 0, grad_out, nullptr, s);
    hipStreamSynchronize(s);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_softmax_argmax(void* stream, const float* logits, float* sm, int64_t* am, int64_t npix, int C)
{ launch_softmax_argmax(logits, sm, (long long*)am, npix, C, (hipStream_t)stream); OPCHK(); return FCN8S_OK; }
int fcn8s_op_confusion(void* stream, const uint8_t* labels, const int64_t* pred, int64_t npix, int64_t* conf, int C)
{ launch_confusion(labels, (const long long*)pred, npix, (unsigned long long*)conf, C, (hipStream_t)stream); OPCHK(); return FCN8S_OK; }
size_t fcn8s_op_cityscapes_work_bytes(int N) { return cityscapes_work_bytes(N); }
int fcn8s_op_cityscapes_pair(void* stream, const uint8_t* gt_label_ids, const uint16_t* gt_instance_ids, const void* pred, int pred_kind,
                             int N, int64_t P, int64_t* conf, void* work, int32_t* entries, int max_entries, int64_t* counts)
{
    if (!gt_label_ids || !pred || !conf || !counts || (pred_kind != 0 && pred_kind != 1) || N <= 0 || P <= 0 || max_entries < 0
        || (gt_instance_ids && (!entries || !work || (uintptr_t)work % 16)))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "cityscapes_pair: bad argument (null pointer, pred_kind outside {0, 1}, N, P <= 0, max_entries < 0, or an instance map without entries / 16-byte aligned work)");
    if (P >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "cityscapes_pair: an image has to have fewer than 2^31 pixels (32-bit counts per instance)");
    take_deferred_error(nullptr);
    launch_cityscapes_pair(gt_label_ids, gt_instance_ids, pred, pred_kind, N, P, (unsigned long long*)conf, work, entries, max_entries,
                           (unsigned long long*)counts, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_reliability_pair(void* stream, const float* prob, const uint8_t* gt, const uint8_t* lut, int N, int64_t P, int C,
                              const float* const* scores, const float* scales, int J, int B,
                              int64_t* calib, int64_t* sums, int64_t* hist, int64_t* bad)
{
    bool ok = prob && gt && lut && calib && sums && hist && bad && N > 0 && P > 0 && C >= 2 && B >= 1 && B <= 64 && J >= 0 && J <= 3
              && (J == 0 || (scores && scales));
    for (int j = 0; ok && j < J; ++j) ok = scores[j] && std::isfinite(scales[j]) && scales[j] > 0.f;
    if (!ok)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "reliability_pair: bad argument (null pointer, N, P <= 0, C < 2, B outside 1 .. 64, J outside 0 .. 3, or a scale that is not finite and positive)");
    if (P >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "reliability_pair: an image has to have fewer than 2^31 pixels");
    take_deferred_error(nullptr);
    launch_reliability_pair(prob, gt, lut, scores, scales, J, N, P, C, B, (unsigned long long*)calib, (unsigned long long*)sums,
                            (unsigned long long*)hist, (unsigned long long*)bad, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
static bool temperature_beta_ok(float b) { return std::isfinite(b) && b >= 0.015625f && b <= 64.f; }
int fcn8s_op_temperature_nll(void* stream, const float* prob, const uint8_t* gt, const uint8_t* lut, int N, int64_t P, int C,
                             const float* betas, int K, int64_t* nll, int64_t* count, int64_t* bad)
{
    bool ok = prob && gt && lut && betas && nll && count && bad && N > 0 && P > 0 && C >= 2 && K >= 1 && K <= FCN8S_TS_MAX_CANDIDATES;
    for (int k = 0; ok && k < K; ++k) ok = temperature_beta_ok(betas[k]);
    if (!ok)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "temperature_nll: bad argument (null pointer, N, P <= 0, C < 2, K outside 1 .. 32, or a beta that is not finite or outside [2^-6, 2^6])");
    if (P >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "temperature_nll: an image has to have fewer than 2^31 pixels");
    take_deferred_error(nullptr);
    launch_temperature_nll(prob, gt, lut, N, P, C, betas, K, (unsigned long long*)nll, (unsigned long long*)count, (unsigned long long*)bad,
                           (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_temperature_apply(void* stream, const float* prob, int N, int64_t P, int C, float beta, float* out, float* entropy_out)
{
    if (!prob || (!out && !entropy_out) || N <= 0 || P <= 0 || C < 2 || !temperature_beta_ok(beta))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "temperature_apply: bad argument (null prob, both outputs null, N, P <= 0, C < 2, or a beta that is not finite or outside [2^-6, 2^6])");
    if (P >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "temperature_apply: an image has to have fewer than 2^31 pixels");
    take_deferred_error(nullptr);
    launch_temperature_apply(prob, N, P, C, beta, out, entropy_out, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_pseudo_label(void* stream, const float* prob, int N, int64_t P, int C, const float* thresholds, const uint8_t* out_ids, int ignore_id,
                          const uint8_t* base, int base_fill, const float* score, float score_max, uint8_t* labels_out,
                          int64_t* hist, int64_t* counts, int64_t* misc)
{
    if (!prob || !counts || !misc || (!labels_out && !hist) || N <= 0 || P <= 0 || C < 2 || C > 255 || ignore_id < 0 || ignore_id > 255
        || base_fill < 0 || base_fill > 255 || (base && !labels_out) || !std::isfinite(score_max))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "pseudo_label: bad argument (null prob / counts / misc, labels_out and hist both null, N, P <= 0, C outside 2 .. 255, ignore_id or base_fill outside 0 .. 255, base without labels_out, or a score_max that is not finite)");
    if (P >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "pseudo_label: an image has to have fewer than 2^31 pixels");
    take_deferred_error(nullptr);
    launch_pseudo_label(prob, N, P, C, thresholds, out_ids, ignore_id, base, base_fill, score, score_max, labels_out,
                        (unsigned long long*)hist, (unsigned long long*)counts, (unsigned long long*)misc, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
size_t fcn8s_op_class_mix_work_bytes(int N) { return class_mix_work_bytes(N); }
int fcn8s_op_class_mix(void* stream, const uint8_t* images, const uint8_t* labels, const int32_t* src, int N, int64_t P, int C, uint64_t seed, uint64_t draw,
                       void* work, uint8_t* out_images, uint8_t* out_labels, uint8_t* selected_out)
{
    if (!images || !labels || !src || !work || !out_images || !out_labels || N <= 0 || P <= 0 || C < 2 || C > 255 || draw >= (1ULL << 48))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "class_mix: bad argument (null images / labels / src / work / out_images / out_labels, N, P <= 0, C outside 2 .. 255, or draw >= 2^48)");
    if (N > 256 || P >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "class_mix: a batch has at most 256 images and an image fewer than 2^31 pixels");
    const uintptr_t T = (uintptr_t)N * (uintptr_t)P;
    const uintptr_t in[3][2] = {{(uintptr_t)images, 3 * T}, {(uintptr_t)labels, T}, {(uintptr_t)src, (uintptr_t)N * 4}};
    const uintptr_t out[2][2] = {{(uintptr_t)out_images, 3 * T}, {(uintptr_t)out_labels, T}};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 3; ++i)
            if (out[o][0] < in[i][0] + in[i][1] && in[i][0] < out[o][0] + out[o][1])
                return fail(nullptr, FCN8S_ERR_BAD_ARG, "class_mix: an output overlaps an input");
    take_deferred_error(nullptr);
    launch_class_mix(images, labels, src, N, P, C, seed, draw, work, out_images, out_labels, selected_out, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
size_t fcn8s_op_entropy_term_work_bytes(void) { return entropy_term_scratch_bytes() + 8; }      // (+ 8: the partials start at the next multiple of 8)
int fcn8s_op_entropy_term(void* stream, const float* logits, float* dlogits, const uint8_t* labels, int N, int64_t HW, int C, int ncols, int pixel_set,
                          int first_image, float weight, void* work, size_t work_bytes, float* term_out, float* bias_out)
{
    if (!logits || !labels || !work || !term_out) return fail(nullptr, FCN8S_ERR_BAD_ARG, "entropy_term: null logits, labels, work or term_out");
    if ((((uintptr_t)logits | (uintptr_t)dlogits | (uintptr_t)term_out | (uintptr_t)bias_out) & 3) != 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "entropy_term: logits, dlogits, term_out and bias_out must be 4-byte aligned");
    if (!std::isfinite(weight)) return fail(nullptr, FCN8S_ERR_BAD_ARG, "entropy_term: the weight must be finite");
    if (C < 2 || C > 64) return fail(nullptr, FCN8S_ERR_BAD_ARG, "entropy_term: C must be in 2 .. 64");
    if (pixel_set < 0 || pixel_set > 2 || ncols < 2 || ncols > C || first_image < 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "entropy_term: pixel_set must be 0, 1 or 2, ncols in 2 .. C and first_image >= 0");
    if (N <= 0 || HW <= 0 || HW > (int64_t)((1LL << 40) / N)) return fail(nullptr, FCN8S_ERR_SHAPE, "entropy_term: N and HW must be positive (and N * HW below 2^40)");
    if (work_bytes < fcn8s_op_entropy_term_work_bytes()) return fail(nullptr, FCN8S_ERR_BAD_ARG, "entropy_term: work is smaller than fcn8s_op_entropy_term_work_bytes()");
    char* ws = (char*)(((uintptr_t)work + 7) & ~(uintptr_t)7);
    take_deferred_error(nullptr);
    launch_entropy_term(logits, dlogits, labels, nullptr, N, (long long)N * HW, C, ncols, pixel_set, first_image, weight, ws, nullptr, term_out, bias_out, 0,
                        (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
size_t fcn8s_op_focal_xent_work_bytes(void) { return focal_xent_scratch_bytes() + 8; }          // (+ 8: the partials start at the next multiple of 8)
int fcn8s_op_focal_xent(void* stream, const float* logits, const uint8_t* labels, const float* class_weights_dev, const uint8_t* codes_dev,
                        const float* table256_dev, float gamma, float* dlogits, float* loss_dev, float* bias_out, int64_t npix, int C, void* work,
                        size_t work_bytes)
{
    if (!logits || !labels || !loss_dev || !work) return fail(nullptr, FCN8S_ERR_BAD_ARG, "focal_xent: null logits, labels, loss_dev or work");
    if ((((uintptr_t)logits | (uintptr_t)class_weights_dev | (uintptr_t)table256_dev | (uintptr_t)dlogits | (uintptr_t)loss_dev | (uintptr_t)bias_out) & 3) != 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "focal_xent: logits, class weights, table, dlogits, loss_dev and bias_out must be 4-byte aligned");
    if (!std::isfinite(gamma) || !(gamma > 0.f) || gamma > 8.f)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "focal_xent: gamma must be in (0, 8] (gamma 0 is the plain cross-entropy: fcn8s_op_softmax_xent, _ex, _px)");
    if (C < 2 || C > 64) return fail(nullptr, FCN8S_ERR_BAD_ARG, "focal_xent: C must be in 2 .. 64");
    if (!codes_dev != !table256_dev) return fail(nullptr, FCN8S_ERR_BAD_ARG, "focal_xent: codes and table must both be given or both be NULL");
    if (npix <= 0 || npix > (1LL << 40)) return fail(nullptr, FCN8S_ERR_SHAPE, "focal_xent: npix must be positive (and at most 2^40)");
    if (work_bytes < fcn8s_op_focal_xent_work_bytes()) return fail(nullptr, FCN8S_ERR_BAD_ARG, "focal_xent: work is smaller than fcn8s_op_focal_xent_work_bytes()");
    char* ws = (char*)(((uintptr_t)work + 7) & ~(uintptr_t)7);
    take_deferred_error(nullptr);
    launch_focal_xent(logits, dlogits, labels, class_weights_dev, codes_dev, table256_dev, nullptr, 1, (long long)npix, C, gamma, 1.0f / (float)npix, ws, nullptr,
                      loss_dev, nullptr, bias_out, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
size_t fcn8s_op_strong_augment_work_bytes(int N) { return strong_augment_work_bytes(N); }
int fcn8s_op_strong_augment(void* stream, const uint8_t* images, int N, int H, int W, uint64_t seed, uint64_t draw, const int32_t* jitter, const int32_t* blur,
                            const uint16_t* taps, void* work, uint8_t* out_images, int32_t* params_out)
{
    if (!images || !work || !out_images || N <= 0 || H <= 0 || W <= 0 || draw >= (1ULL << 48))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "strong_augment: bad argument (null images / work / out_images, N, H or W <= 0, or draw >= 2^48)");
    if (jitter && (jitter[0] < 0 || jitter[0] > 65536 || jitter[1] < 0 || jitter[1] > 65536 || jitter[2] < 0 || jitter[2] > 65536 || jitter[3] < 0 ||
                   jitter[3] > 65536 || jitter[4] < 0 || jitter[4] > 90))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "strong_augment: jitter is {gate 0..65536, contrast, saturation, brightness 0..65536, hue 0..90}");
    if (blur) {
        if (blur[0] < 0 || blur[0] > 65536 || blur[1] < 1 || blur[1] > 16 || blur[2] < 1 || blur[2] > 7 || !taps)
            return fail(nullptr, FCN8S_ERR_BAD_ARG, "strong_augment: blur is {gate 0..65536, levels 1..16, radius 1..7} and needs taps");
        for (int q = 0; q < blur[1]; ++q) {
            const uint16_t* w = taps + q * (blur[2] + 1);
            int sum = w[0];
            for (int i = 1; i <= blur[2]; ++i) {
                if (w[i] > w[i - 1]) return fail(nullptr, FCN8S_ERR_BAD_ARG, "strong_augment: a row of taps increases");
                sum += 2 * w[i];
            }
            if (sum != 2048) return fail(nullptr, FCN8S_ERR_BAD_ARG, "strong_augment: a row of taps does not sum to 2048 (w[0] + 2 (w[1] + ... + w[R]))");
        }
    }
    if (N > 256 || (int64_t)H * W >= (1LL << 31))
        return fail(nullptr, FCN8S_ERR_SHAPE, "strong_augment: a batch has at most 256 images and an image fewer than 2^31 pixels");
    if (blur && (H <= blur[2] || W <= blur[2])) return fail(nullptr, FCN8S_ERR_SHAPE, "strong_augment: the blur needs H > R and W > R (one reflection)");
    const uintptr_t T = (uintptr_t)N * (uintptr_t)H * (uintptr_t)W * 3;
    if ((uintptr_t)out_images < (uintptr_t)images + T && (uintptr_t)images < (uintptr_t)out_images + T)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "strong_augment: out_images overlaps images (the blur reads neighbours: not in place)");
    take_deferred_error(nullptr);
    launch_strong_augment(images, N, H, W, seed, draw, jitter, blur, taps, work, out_images, params_out, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
size_t fcn8s_op_fda_work_bytes(int N, int M, int H, int W, int b) { return fda_work_bytes(N, M, H, W, b); }
int fcn8s_op_fda_transfer(void* stream, const uint8_t* images, int N, const uint8_t* targets, int M, int H, int W, int b, const int32_t* pair_dev, void* work,
                          uint8_t* out_u8, float* out_f32)
{
    if (!images || !targets || !work || (!out_u8 && !out_f32) || N <= 0 || M <= 0 || H <= 0 || W <= 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "fda_transfer: bad argument (null images / targets / work, both outputs null, or N, M, H or W <= 0)");
    if (b < 0 || b > 96 || 2 * b + 1 > (H < W ? H : W))
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "fda_transfer: the half-width b must satisfy 0 <= b <= 96 and 2 b + 1 <= min(H, W)");
    if (((uintptr_t)out_f32 & 3) != 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "fda_transfer: out_f32 must be 4-byte aligned");
    if (N > 256 || M > 256 || (int64_t)H * W >= (1LL << 31))
        return fail(nullptr, FCN8S_ERR_SHAPE, "fda_transfer: a batch has at most 256 images and an image fewer than 2^31 pixels");
    {
        const uintptr_t P3 = (uintptr_t)H * (uintptr_t)W * 3;
        const uintptr_t in[4][2] = {{(uintptr_t)images, (uintptr_t)N * P3}, {(uintptr_t)targets, (uintptr_t)M * P3},
                                    {(uintptr_t)pair_dev, pair_dev ? (uintptr_t)N * 4 : 0}, {(uintptr_t)work, (uintptr_t)fda_work_bytes(N, M, H, W, b)}};
        const uintptr_t out[2][2] = {{(uintptr_t)out_u8, out_u8 ? (uintptr_t)N * P3 : 0}, {(uintptr_t)out_f32, out_f32 ? (uintptr_t)N * P3 * 4 : 0}};
        for (int o = 0; o < 2; ++o)
            for (int i = 0; i < 4; ++i)
                if (out[o][1] && in[i][1] && out[o][0] < in[i][0] + in[i][1] && in[i][0] < out[o][0] + out[o][1])
                    return fail(nullptr, FCN8S_ERR_BAD_ARG, "fda_transfer: an output overlaps images, targets, pair_dev or work");
        if (out[0][1] && out[1][1] && out[0][0] < out[1][0] + out[1][1] && out[1][0] < out[0][0] + out[0][1])
            return fail(nullptr, FCN8S_ERR_BAD_ARG, "fda_transfer: the two outputs overlap");
    }
    take_deferred_error(nullptr);
    launch_fda_transfer(images, N, targets, M, H, W, b, pair_dev, work, out_u8, out_f32, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_boundary_pair(void* stream, const uint8_t* gt_label_ids, const void* pred, int pred_kind, int N, int H, int W, int R,
                           int64_t* rings, int64_t* bprec, int64_t* brec, int64_t* bad)
{
    if (!gt_label_ids || !pred || !rings || !bprec || !brec || !bad || (pred_kind != 0 && pred_kind != 1) || N <= 0 || H <= 0 || W <= 0 || R < 1 || R > 16)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "boundary_pair: bad argument (null pointer, pred_kind outside {0, 1}, N, H, W <= 0, or R outside 1 .. 16)");
    if ((long long)H * W >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "boundary_pair: an image has to have fewer than 2^31 pixels");
    take_deferred_error(nullptr);
    launch_boundary_pair(gt_label_ids, pred, pred_kind, N, H, W, R, (unsigned long long*)rings, (unsigned long long*)bprec, (unsigned long long*)brec,
                         (unsigned long long*)bad, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_boundary_distance(void* stream, const uint8_t* label_ids, int N, int H, int W, int R, uint8_t* codes_out)
{
    if (!label_ids || !codes_out || N <= 0 || H <= 0 || W <= 0 || R < 1 || R > 15)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "boundary_distance: bad argument (null pointer, N, H, W <= 0, or R outside 1 .. 15)");
    if ((long long)H * W >= (1LL << 31)) return fail(nullptr, FCN8S_ERR_SHAPE, "boundary_distance: an image has to have fewer than 2^31 pixels");
    take_deferred_error(nullptr);
    launch_boundary_distance(label_ids, N, H, W, R, codes_out, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
size_t fcn8s_op_regions_work_bytes(int N, int H, int W) { return (long long)H * W >= (1LL << 31) ? 0 : regions_work_bytes(N, H, W); }
static int regions_args(const char* what, const void* labels, int label_kind, int N, int H, int W, int connectivity, const void* work, bool rest_ok)
{
    if (!labels || !work || (uintptr_t)work % 16 || !rest_ok || (label_kind != 0 && label_kind != 1) || (connectivity != 4 && connectivity != 8) || N <= 0 || H <= 0 || W <= 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, std::string(what) + ": bad argument (null pointer, work not 16-byte aligned, label_kind outside {0, 1}, connectivity outside {4, 8}, rounds outside 1 .. 8, or N, H, W <= 0)");
    if ((long long)H * W >= (1LL << 31) || N > 65535) return fail(nullptr, FCN8S_ERR_SHAPE, std::string(what) + ": an image has to have fewer than 2^31 pixels and a batch at most 65535 images");
    return FCN8S_OK;
}
int fcn8s_op_regions_label(void* stream, const void* labels, int label_kind, int N, int H, int W, int connectivity, int32_t* comp_out, int32_t* area_out, void* work)
{
    const int rc = regions_args("regions_label", labels, label_kind, N, H, W, connectivity, work, comp_out != nullptr);
    if (rc) return rc;
    take_deferred_error(nullptr);
    launch_regions_label(labels, label_kind, N, H, W, connectivity, comp_out, area_out, work, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_regions_clean(void* stream, void* labels, int label_kind, int N, int H, int W, int connectivity, const int32_t* min_area_dev, int rounds,
                           void* work, int64_t* stats_dev)
{
    const int rc = regions_args("regions_clean", labels, label_kind, N, H, W, connectivity, work, min_area_dev != nullptr && rounds >= 1 && rounds <= 8);
    if (rc) return rc;
    take_deferred_error(nullptr);
    launch_regions_clean(labels, label_kind, N, H, W, connectivity, min_area_dev, rounds, work, (unsigned long long*)stats_dev, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_regions_status(void* stream, const void* work, int64_t* status_host)
{
    if (!work || !status_host) return fail(nullptr, FCN8S_ERR_BAD_ARG, "regions_status: null pointer");
    long long st[2] = {0, 0};
    if (!regions_status(work, st, (hipStream_t)stream)) return fail(nullptr, FCN8S_ERR_HIP, "regions_status: the header could not be read");
    status_host[0] = st[0]; status_host[1] = st[1];
    return FCN8S_OK;
}
size_t fcn8s_op_panoptic_work_bytes(int N, int64_t slots_per_image) { return panoptic_work_bytes(N, slots_per_image); }
int fcn8s_op_panoptic_pair(void* stream, const uint16_t* gt_instance_ids, const void* pred, int pred_kind, const int32_t* pred_comp, int N, int H, int W,
                           void* work, int64_t slots_per_image, int64_t* rows, int64_t max_rows, int64_t* counts)
{
    if (!gt_instance_ids || !pred || !pred_comp || !work || (uintptr_t)work % 16 || !rows || !counts || (pred_kind != 0 && pred_kind != 1) || N <= 0 || H <= 0 || W <= 0
        || max_rows < 1 || panoptic_work_bytes(N > 0 ? N : 1, slots_per_image) == 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "panoptic_pair: bad argument (null pointer, work not 16-byte aligned, pred_kind outside {0, 1}, N, H, W <= 0, max_rows < 1, or slots_per_image no power of two in 1 .. 2^28)");
    if ((long long)H * W > (1LL << 26) || N > 65535)
        return fail(nullptr, FCN8S_ERR_SHAPE, "panoptic_pair: an image has to have at most 2^26 pixels (26-bit component ids) and a batch at most 65535 images");
    take_deferred_error(nullptr);
    launch_panoptic_pair(gt_instance_ids, pred, pred_kind, pred_comp, N, H, W, work, slots_per_image, (long long*)rows, max_rows, (unsigned long long*)counts,
                         (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
size_t fcn8s_op_instance_work_bytes(int N, int64_t slots_per_image) { return instance_work_bytes(N, slots_per_image); }
int fcn8s_op_instance_pair(void* stream, const float* prob, int C, const uint8_t* labels, const int32_t* comp, const uint16_t* gt_instance_ids, int N, int H, int W,
                           void* work, int64_t slots_per_image, int64_t* rows, int64_t max_rows, int64_t* counts)
{
    if (!prob || !labels || !comp || !work || (uintptr_t)work % 16 || (uintptr_t)prob % 4 || !rows || !counts || C < 20 || N <= 0 || H <= 0 || W <= 0
        || max_rows < 1 || instance_work_bytes(N > 0 ? N : 1, slots_per_image) == 0)
        return fail(nullptr, FCN8S_ERR_BAD_ARG, "instance_pair: bad argument (null pointer, work not 16-byte aligned, C < 20, N, H, W <= 0, max_rows < 1, or slots_per_image no power of two in 1 .. 2^28)");
    if ((long long)H * W > (1LL << 26) || N > 65535 || (long long)C * 4 > (1LL << 20))
        return fail(nullptr, FCN8S_ERR_SHAPE, "instance_pair: an image has to have at most 2^26 pixels (26-bit component ids), a batch at most 65535 images and a row at most 2^18 classes");
    take_deferred_error(nullptr);
    launch_instance_pair(prob, C, labels, comp, gt_instance_ids, N, H, W, work, slots_per_image, (long long*)rows, max_rows, (unsigned long long*)counts,
                         (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
// the six op-level forms of the update: host scale or the slab's (out5 + 2: s, out5 + 3: ok), with or without a shadow
static int op_update(void* stream, int opt, float* theta, const float* g, float* m, float* v, float* shadow, int64_t n,
                     float p0, float p1, float p2, float p3, float gs, const float* out5, float w)
{
    launch_update({ opt, theta, g, m, v, shadow, n, p0, p1, p2, p3, gs, out5 ? out5 + 2 : nullptr, out5 ? (const int*)(out5 + 3) : nullptr, w }, (hipStream_t)stream);
    OPCHK(); return FCN8S_OK;
}
int fcn8s_op_tf_adam(void* stream, float* theta, const float* g, float* mm, float* v, int64_t n, int t, float lr, float b1, float b2, float eps, float gs)
{ return op_update(stream, FCN8S_OPT_TF_ADAM, theta, g, mm, v, nullptr, n, tf_adam_lr_t(lr, b1, b2, t), b1, b2, eps, gs, nullptr, 0.f); }
int fcn8s_op_sgd_momentum(void* stream, float* theta, const float* g, float* buf, int64_t n, float lr, float mom, float gs)
{ return op_update(stream, FCN8S_OPT_SGD_MOMENTUM, theta, g, buf, nullptr, nullptr, n, lr, mom, 0.f, 0.f, gs, nullptr, 0.f); }
int fcn8s_op_grad_accumulate(void* stream, float* dst, const float* src, int64_t n, int mode)
{
    if (!dst || !src || n < 0 || (mode != 0 && mode != 1)) return fail(nullptr, FCN8S_ERR_BAD_ARG, "grad_accumulate: bad argument (null pointer, n < 0, or mode outside {0, 1})");
    launch_grad_accumulate(dst, src, n, mode, (hipStream_t)stream); OPCHK(); return FCN8S_OK;
}
int fcn8s_op_grad_norm(void* stream, const float* g, int64_t n, float grad_scale, float max_norm, float* out5_dev)
{
    if (!g || !out5_dev || n < 0 || !(max_norm >= 0.f)) return fail(nullptr, FCN8S_ERR_BAD_ARG, "grad_norm: bad argument (null pointer, n < 0, or max_norm negative / NaN)");
    DeviceBuf<double> partials;                          // (freed on return: behind the stream's synchronise)
    if (!partials.grow(kGradNormBlocks * sizeof(double), (hipStream_t)stream)) return fail(nullptr, FCN8S_ERR_OOM, "grad_norm: out of device memory");
    launch_grad_norm(g, n, grad_scale, max_norm, partials, out5_dev, true, (hipStream_t)stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, FCN8S_ERR_HIP, hipGetErrorString(e));
    OPCHK(); return FCN8S_OK;
}
// (out5_dev[3] is 1.0f or 0.0f: as an int it is non-zero exactly when the guard said ok)
int fcn8s_op_tf_adam_dev(void* stream, float* theta, const float* g, float* mm, float* v, int64_t n, int t, float lr, float b1, float b2, float eps, const float* out5)
{
    if (!out5) return fail(nullptr, FCN8S_ERR_BAD_ARG, "tf_adam_dev: null out5_dev");
    return op_update(stream, FCN8S_OPT_TF_ADAM, theta, g, mm, v, nullptr, n, tf_adam_lr_t(lr, b1, b2, t), b1, b2, eps, 0.f, out5, 0.f);
}
int fcn8s_op_sgd_momentum_dev(void* stream, float* theta, const float* g, float* buf, int64_t n, float lr, float mom, const float* out5)
{
    if (!out5) return fail(nullptr, FCN8S_ERR_BAD_ARG, "sgd_momentum_dev: null out5_dev");
    return op_update(stream, FCN8S_OPT_SGD_MOMENTUM, theta, g, buf, nullptr, nullptr, n, lr, mom, 0.f, 0.f, 0.f, out5, 0.f);
}
int fcn8s_op_ema_update(void* stream, float* s, const float* theta, int64_t n, float w, const float* out5)
{
    if (!s || !theta || n < 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "ema_update: bad argument (null pointer or n < 0)");
    launch_ema_update(s, theta, n, w, out5 ? (const int*)(out5 + 3) : nullptr, (hipStream_t)stream); OPCHK(); return FCN8S_OK;
}
int fcn8s_op_tf_adam_ema(void* stream, float* theta, const float* g, float* mm, float* v, float* s, int64_t n, int t, float lr, float b1, float b2, float eps,
                         float gs, const float* out5, float w)
{
    if (!theta || !g || !mm || !v || !s || n < 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "tf_adam_ema: bad argument (null pointer or n < 0)");
    return op_update(stream, FCN8S_OPT_TF_ADAM, theta, g, mm, v, s, n, tf_adam_lr_t(lr, b1, b2, t), b1, b2, eps, gs, out5, w);
}
int fcn8s_op_sgd_momentum_ema(void* stream, float* theta, const float* g, float* buf, float* s, int64_t n, float lr, float mom, float gs, const float* out5, float w)
{
    if (!theta || !g || !buf || !s || n < 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "sgd_momentum_ema: bad argument (null pointer or n < 0)");
    return op_update(stream, FCN8S_OPT_SGD_MOMENTUM, theta, g, buf, nullptr, s, n, lr, mom, 0.f, 0.f, gs, out5, w);
}
int fcn8s_op_swap(void* stream, float* a, float* b, int64_t n)
{
    if (!a || !b || n < 0) return fail(nullptr, FCN8S_ERR_BAD_ARG, "swap: bad argument (null pointer or n < 0)");
    launch_swap(a, b, n, (hipStream_t)stream); OPCHK(); return FCN8S_OK;
}

}  // extern "C"
