// Internal launcher interface shared by the HIP translation units.
// gfx950 only.  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "../../include/fcn8s_hip.h"      // the status codes (defer_error)

// gfx950 (MI355X, CDNA4) only: the kernels rely on 160 KB of LDS per workgroup (conv_bf16_256_kernel: five 32 KB stages; wino_out_in_kernel: 96 KB
// static), on global_load_lds_dwordx4, ds_read_b64_tr_b16 and the gfx950 MFMA shapes.  A device pass for any other target stops here with a
// readable message instead of "local memory limit exceeded" deep inside a template; fcn8s_create checks the same thing at run time.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libfcn8s_hip is written for gfx950 (MI355X) only: build with --offload-arch=gfx950"
#endif
#define FCN8S_LDS_BYTES_NEEDED (160u * 1024u)

#include <string>
namespace fcn8s {

// symbol of the MFMA kernel the last launch_* call used (for the per-kernel profile view)
extern thread_local const char* g_last_kernel;
// A launcher that cannot run -- a shape no kernel of the chosen arithmetic takes, a scratch allocation that failed, a broken internal promise -- records why and
// returns WITHOUT launching; the C entry point that called it (fcn8s_forward_loss, fcn8s_backward_bucket, fcn8s_predict, ..., every fcn8s_op_*) then returns `code`
// with the text in fcn8s_last_error instead of the process dying in abort() (in a data-parallel run an aborted rank also cost its peers a full watchdog timeout).
// The first error wins; the slot belongs to the calling thread.
void defer_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int take_deferred_error(std::string* text);       // the recorded code (0: none) and its text; clears the slot

// ---------------------------------------------------------------------------
// Implicit-GEMM convolution on the f32 MFMA (v_mfma_f32_32x32x2_f32).
//
//   Y[m, j] = epilogue( alpha * sum_{tap, c} X[src(m, tap), c] * W[tap*Cin + c, j] )
//
// m runs over an (N, Ma, Mb) grid.  src(m,tap) = (n, in_scale*a + dy, in_scale*b + dx),
// (dy,dx) = (ty,tx)*tap_step + tap_off, zero outside [0,Hi)x[0,Wi).
// The output row of m is pixel (n, out_scale*a + out_offy, out_scale*b + out_offx)
// of an (N,Ho,Wo,ldy) tensor; rows falling outside are not stored.
// gridDim.z enumerates "phases" (transposed-conv sub-pixel phases): phase z uses
// weights w + z*w_phase_stride and adds (z / phases_x, z % phases_x) to the output offsets.
// One parameterisation therefore covers: 3x3 / 7x7 / 1x1 SAME convs, their data
// gradients (flipped+transposed weights), the strided conv that is the data
// gradient of a transposed conv, and the transposed conv itself (s*s phases of 2x2 convs).
// ---------------------------------------------------------------------------
struct IgemmArgs {
    const float* x; const float* w; const float* bias; const float* addend; const float* mask;
    float* y;
    int N, Ma, Mb; long long M;
    int Hi, Wi, Cin, ldx;
    int KW, in_scale, tap_step, tap_off, Ktot;
    int Ho, Wo, Cout, ldy;
    int out_scale, out_offy, out_offx;
    int phases_x; long long w_phase_stride;
    float alpha; int relu; float mask_scale;
    int dropout; float keep_prob; unsigned long long seed; unsigned int stream_id;
    int batched; long long x_batch_stride, y_batch_stride;   // gridDim.z independent GEMMs (Winograd positions)
    int m_fastest;                                           // tile order, set by the launcher (see igemm.hip)
    int bt, ldw;                                             // bt: the B operand is stored transposed, w[z][n][k] with row stride ldw (plain batched GEMMs on the LDS-DMA kernel only)
    int fixed_tile;                                          // 1: 128-row tiles (128 columns, 64 if Cout % 128), never split-K -- the choice depends on the caller's per-image geometry, not on M
    int split;                                               // 3: the LDS-DMA kernels take their products as six bf16 MFMAs of the operands split in three (FCN8S_PREC_F32X3); 2: three MFMAs of two pieces (FCN8S_PREC_F32X2); 0: f32 MFMA
};
void launch_igemm(const IgemmArgs& a, int phases, hipStream_t s);

// ---------------------------------------------------------------------------
// bf16-operand / fp32-accumulate SAME conv (stride 1, odd K) on v_mfma_f32_32x32x16_bf16 -- the optional fc6 / fc7
// precision mode (gemm_bf16.hip).  x: fp32 NHWC; wt: bf16 K-tile-major blocks written by launch_w_to_bf16_tiles from the
// fp32 HWIO kernel; y: fp32.  Needs Cin % 32 == 0, Cout % 128 == 0 (launch returns false otherwise).
// ---------------------------------------------------------------------------
struct Bf16ConvArgs {
    const float* x; const unsigned short* xh;   // activations: fp32, or (xh != nullptr) already converted by launch_f32_to_bf16
    const unsigned short* wt; const float* bias; float* y;
    int N, H, W, Cin, Cout, K;
    int relu, dropout; float keep_prob; unsigned long long seed; unsigned int stream_id;
    long long M; int m_fastest;        // filled in by the launcher
};
void launch_w_to_bf16_tiles(const float* w, unsigned short* wt, int K, int Cout, hipStream_t s);   // w[K][Cout] -> wt[K/32][Cout][32]
bool launch_conv_bf16(const Bf16ConvArgs& a, hipStream_t s);
void launch_f32_to_bf16(const float* x, unsigned short* y, long long n, hipStream_t s);                // n % 8 == 0
// 256 x 256 tile variant (gemm_bf16.hip): zero-padded bf16 activations [N][H + K - 1][W + K - 1][Cin], kernel transposed to wt[Cout][K*K*Cin] bf16
struct Bf16Conv256Args {
    const unsigned short* xp; const unsigned short* wt; const float* bias; float* y;
    int N, H, W, Cin, Cout, K;
    int relu, dropout; float keep_prob; unsigned long long seed; unsigned int stream_id;
    long long M; int m_fastest;        // filled in by the launcher
    const float* addend;               // optional, [M][Cout]: added before ReLU / mask (a data gradient's skip-path term)
    const float* mask; float mask_scale;   // optional, [M][Cout]: y = mask > 0 ? y * mask_scale : 0 (the ReLU / dropout of the layer whose input gradient this is)
    int any_shape;                     // 1: Cout % 64 == 0 and any M are taken (64- / 128-column tiles, partial last row tile); 0: the round-3 rule
    const unsigned short* mask16;      // optional (flat-position kernel only): the padded bf16 copy [N][H + 2][W + 2][Cout] whose sign is the mask, instead of `mask`
    float* colpart;                    // optional (flat-position kernel only): [row tiles][Cout] column sums of the tile's stored values, one row per row tile
    int ksplit; float* part;           // set by the launcher: K split over blockIdx.y into `ksplit` slabs of raw accumulators at `part`
    int rows_bn;                       // (A/B) 128: the flat-position kernel takes its 128-column form where Cout % 128 == 0 (default: 64 columns everywhere)
    int guarded;                       // 1: xp has zeroed guard rows in front and behind (>= W + 3 + 16 rows of Cin): the flat-position kernel may be taken
    unsigned short* yb; int yb_pad;    // optional: also write the output as bf16 into the interior of a padded copy [N][H + 2 yb_pad][W + 2 yb_pad][Cout] (points at its pixel 0)
    // Channel-chunk PLANES (bf16_train's per-layer copies): a padded copy may be stored as [C / 32][rows][32] instead of [rows][C] -- the 64-byte slice (one
    // position, 32 channels) that is one LDS row of a K-tile then lies next to its neighbour positions' slices and an LDS-DMA instruction reads 1 KB of contiguous
    // memory, whole 128-byte lines, instead of sixteen half lines.  *_ps = elements between two planes ((rows + guard rows) * 32); 0 = [rows][C].  The pointers
    // point at padded pixel 0 of plane 0.
    long long xp_ps, yb_ps, mask16_ps;
};
bool conv_bf16_256_ok(long long M, int Cin, int Cout, int mode);      // mode 0 never, 1 when it fills the chip, 2 whenever the shapes allow
void launch_w_to_bf16_t(const float* w, unsigned short* wt, int K, int Cout, hipStream_t s);
void launch_f32_to_bf16_padded(const float* x, unsigned short* xp, int N, int H, int W, int C, int pad, hipStream_t s, long long ps = 0);      // ps: plane stride of xp in elements, 0 = [rows][C]
int conv_bf16_rows_bm(int Cout, int rows_bn);      // positions per row tile (= per partial row of `colpart`) of the form launch_conv_bf16_256 picks
bool launch_conv_bf16_256(const Bf16Conv256Args& a, hipStream_t s);
// FCN8S_PREC_FP8_INFER (gemm_fp8.hip): e4m3 convolution on the MX MFMA.  xp: padded e4m3 copy of the input, pixel 0 of plane 0, 64-channel planes
// xp_ps bytes apart (pad (K - 1) / 2); wq: [K K Cin / 64][Cout][64] e4m3 with per-column exponents ew; y = 2^(ex + ew) sum Xq Wq + bias (ReLU).
// y (fp32 [M][Cout]) and / or yq (the consumer's padded copy: pad yq_pad, planes yq_ps bytes apart, q(y 2^-yq_exp)) may be NULL.  Cin, Cout % 64 == 0.
struct Fp8ConvArgs {
    const unsigned char* xp = nullptr; long long xp_ps = 0;
    const unsigned char* wq = nullptr; const int* ew = nullptr;
    const float* bias = nullptr; float* y = nullptr;
    unsigned char* yq = nullptr; long long yq_ps = 0; int yq_pad = 0, yq_exp = 0;
    int ex = 0, relu = 1;
    int N = 0, H = 0, W = 0, Cin = 0, Cout = 0, K = 1;
    long long M = 0;
};
bool launch_conv_fp8(const Fp8ConvArgs& a, hipStream_t s);
void launch_w_to_fp8(const float* w, unsigned char* wq, int* ew, unsigned* amax_scratch, int rows, int Cout, hipStream_t s);
void launch_f32_to_fp8_padded(const float* x, unsigned char* xq, int N, int H, int W, int C, int pad, long long ps, int ex, hipStream_t s);
void launch_zero_border_fp8(unsigned char* xq, int planes, long long ps, int N, int H, int W, int pad, hipStream_t s);
void launch_maxpool_fp8(const unsigned char* xq, long long xps, unsigned char* yq, long long yps, int N, int H, int W, int C, int ypad, hipStream_t s);
void launch_amax(const float* x, long long n, unsigned* amax, hipStream_t s);
// the padded bf16 copy of an output gradient (interior only: the border of xp is zero already) with db[c] += column sums of x on the way
bool launch_f32_to_bf16_padded_colsum(const float* x, unsigned short* xp, float* db, int N, int H, int W, int C, int pad, hipStream_t s, long long ps = 0);
// the kernel of a SAME convolution's data gradient as conv_bf16_256_kernel wants it: wt[Cin][(flipped taps, Cout)] bf16 (Cout % 8 == 0)
void launch_w_to_bf16_flip_t(const float* w, unsigned short* wt, int K, int Cin, int Cout, hipStream_t s);
// weight gradient with bf16-rounded operands: dW[tap][ci][co] = sum_q A[q + off(tap)][ci] * B[q][co] over R flat padded-pixel rows (gemm_bf16.hip)
struct Bf16WgradArgs {
    const unsigned short* A; const unsigned short* B; float* C;      // A = padded bf16 input [R][Ci], B = padded bf16 output gradient [R][Cj], both with guard rows
    long long R; int Ci, Cj, K, Wp;                                   // R = N * Hp * Wp, Wp = W + K - 1
    long long chunk, split_stride; int plain_store;                   // set by the launcher
    long long a_ps, b_ps;                                             // channel-chunk planes (see Bf16Conv256Args): elements between two 32-channel planes of A / B, 0 = [R][C]
};
bool launch_wgrad_bf16(const Bf16WgradArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// Weight-gradient GEMM on the f32 MFMA:
//   C[tap][i][j] += alpha * sum_p A[srcA(p, tap), i] * B[p, j]
// p runs over the (N, Pa, Pb) pixel grid of B; srcA = (n, a_scale*a + dy, a_scale*b + dx).
// Split over p across gridDim.y with float atomics into a zero-initialised C.
// ---------------------------------------------------------------------------
struct WgradArgs {
    const float* A; const float* B; float* C;
    int N, Pa, Pb; long long P;
    int Ha, Wa, Adim, lda, Areal;      // A tensor (N,Ha,Wa,lda); Adim channels loadable (mult of 4); Areal rows stored
    int Bdim, ldb;                     // B tensor (N,Pa,Pb,ldb); Bdim channels (mult of 4)
    int KW, a_scale, tap_off, ntaps;   // dy = ty + tap_off
    int ldc;                           // C[tap] is [Areal][ldc]
    float alpha;
    float* colsum;                     // optional: colsum[j] += sum_p B[p,j]  (bias gradient), or nullptr
    int batched; long long a_batch_stride, b_batch_stride;   // gridDim.z = independent GEMMs (C stride = Areal*ldc)
    int c_uninitialized;               // 0: C was zeroed by the caller (accumulate with atomics); 1: the launcher decides (plain store or memset)
    int plain_store;                   // set by the launcher
    int split;                         // as IgemmArgs::split
    long long split_stride;            // set by the launcher (deterministic mode): != 0 = reduction split k stores its partial tile at C + k * split_stride
};
void launch_wgrad(const WgradArgs& a, hipStream_t s);

// ---- deterministic mode (model option "deterministic") ---------------------------------------------------------------
// Every reduction that the default path splits over blocks and joins with fp32 atomics (weight gradients, bias gradients: the order of the
// additions then depends on block scheduling, so no two runs give the same bits) instead stores one partial result per split into a scratch slab
// and a second kernel adds the slabs in split order.  Set per thread by the model's entry points; launchers read it.
extern thread_local int t_deterministic;
float* det_scratch(hipStream_t s, size_t floats);              // per-(device, stream) scratch, grown on demand; nullptr if the allocation failed
float* scratch2(hipStream_t s, size_t floats);                 // a second such buffer (the column sums' partials, which run beside a det_scratch user)
void scratch_release(hipStream_t s);                           // frees both buffers of the calling device's stream s (fcn8s_destroy; the stream is idle)
// op context "op_poison_scratch" (tests; 0 everywhere else): every hand-out of the two pools is filled with 0xFF bytes on the caller's stream, so a
// producer and its consumer must sit under ONE hand-out (they do at all ten call sites: a det_scratch user that ends in launch_colsum meets
// scratch2, the other pool).  t_scratch_poisoned_bytes: what has been filled since the option was last set ("op_scratch_poisoned_bytes").
extern thread_local int t_poison_scratch;
extern thread_local long long t_scratch_poisoned_bytes;
long long scratch_bytes_live();                                // bytes the two per-(device, stream) pools hold right now, all devices and streams (option "scratch_bytes_live")
// C[r][c] (= or +=) sum_{k < nsplit, in order} ws[k * slab + r * ldc + c]   for r < rows, c < cols
void launch_det_reduce(float* C, const float* ws, long long rows, int cols, int ldc, long long slab, int nsplit, bool accumulate, hipStream_t s);
// 3x3 / 7x7 SAME conv weight (+bias) gradient, several taps per block (3x3: all nine, 7x7: one filter row);
// returns false if the shape is not covered (K, Cin % 64, Cout % 64, W % 16): the caller then uses launch_wgrad.
bool launch_wgrad_taps(const float* X, const float* dZ, float* dW, float* db, int N, int H, int W, int Cin, int Cout,
                       int K, hipStream_t s);

// conv1_1 (3 -> 64 channels, 4-channel padded input) weight + bias gradient, VALU, HBM-bound;
// returns false if the shape is not covered (Cout != 64 or W % 64).
bool launch_conv1_wgrad(const float* X4, const float* dZ, float* dW, float* db, int N, int H, int W, int Cout, int mfma, hipStream_t s);

// conv1_1 forward with bias + ReLU on the LDS-DMA gather kernel (Cout = 64 only; returns false otherwise): x4 [N,H,W,4], w48 [48][64]
// (taps x 4 channels, rows 36..47 zero), zero16 = 16 zero bytes in device memory (what taps outside the image read)
bool launch_conv1_fwd(const float* x4, const float* w48, const float* bias, float* y, const float* zero16, int N, int H, int W, int Cout, int tiled, hipStream_t s, unsigned short* yb16 = nullptr, long long yb16_ps = 0);

// weight gradient of the 16x16 / stride-8 transposed conv with 20 channels (VALU; dW zero-initialised, accumulated with atomics);
// returns false for any other shape: the caller then uses launch_wgrad.
bool launch_tconv_wgrad(const float* X, const float* dY, float* dW, int N, int Hi, int Wi, int C, int K, int S, hipStream_t s);

// ---------------------------------------------------------------------------
// Element-wise / reduction kernels (HBM-bound)
// ---------------------------------------------------------------------------
void launch_preprocess(const void* img, int dtype, float* out4, long long npix, hipStream_t s);
void launch_maxpool_fwd(const float* x, float* y, int N, int H, int W, int C, hipStream_t s);
void launch_maxpool_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C,
                        int relu_mask, hipStream_t s);
void launch_maxpool_route(const float* x, unsigned char* route, int N, int H, int W, int C, hipStream_t s);
void launch_maxpool_fwd_route(const float* x, float* y, unsigned char* r, int N, int H, int W, int C, hipStream_t s, unsigned short* yb16 = nullptr, int pad = 0, long long yb16_ps = 0, int round16 = 0);
// ... the same over the block's last activation kept only as its bf16 copy (channel-chunk planes of the zero-bordered map, plane stride xb_ps); yb16 likewise
void launch_maxpool_fwd_route16(const unsigned short* xb, long long xb_ps, unsigned char* r, int N, int H, int W, int C, hipStream_t s, unsigned short* yb16, int pad, long long yb16_ps);   // forward pool + those bytes in one pass
// Where the logits of pixel slot p live.  blocked == 0: slot = pixel, NHWC.  blocked != 0: the layout the last transposed conv
// (k = 2s, stride s, pad s/2) produces when it runs as ONE GEMM (model.hip: tconv_gemm_*): rows = (n, q, qx) over an (H/s + 1) x (W/s + 1)
// grid of s x s output blocks that start at pixel (s q - s/2, s qx - s/2), columns = (r, rx, class); slots of the half blocks that
// stick out of the image exist but are invalid (their gradient is written as 0).
struct PixMap { int blocked, H, W, QH, QW, S; };
static __host__ __device__ inline long long pixmap_slots(const PixMap& m, long long npix, int N) { return m.blocked ? (long long)N * m.QH * m.QW * m.S * m.S : npix; }
// partials: double[>= softmax_xent_blocks(npix)]
int  softmax_xent_blocks(long long npix);
void launch_softmax_xent(const float* logits, const uint8_t* labels, float* dlogits, double* partials,
                         long long npix, int C, float grad_scale, hipStream_t s, float* colsum = nullptr,   /* colsum[c] += sum_p dlogits[p,c] (zero-initialised by the caller) */
                         const PixMap* map = nullptr, int N = 0);
// The training loss's class weights and online hard-example mining (fcn8s_set_loss, include/fcn8s_hip.h).  The scratch is LOSS_SCRATCH_BYTES
// of state and histograms (zeroed by launch_softmax_xent_ex) followed, for OHEM, by the pixel-indexed l_p buffer (float[npix]).
enum XentPhase { XENT_PLAIN = 0, XENT_WEIGHTED = 1, XENT_OHEM_LOSS = 2, XENT_OHEM_GRAD = 3 };
struct OhemState {
    unsigned long long valid, ntau, kept;   // |V|, |{l >= tau}|, |K|
    unsigned long long krem, above;         // selection: the rank still sought under the prefix, the keys above it
    unsigned prefix; int active;            // the key bits fixed so far; 1 = the refinement levels run
    float t, gscale;                        // the threshold t and the gradient scale 1 / |K|
    unsigned pad[2];
};
static_assert(sizeof(OhemState) == 64, "OhemState: 64 bytes");
constexpr size_t LOSS_SCRATCH_BYTES = sizeof(OhemState) + (2048 + 2048 + 1024) * sizeof(unsigned);
struct XentEx {
    const float* cw = nullptr;             // class weights, device float[C]
    float* lbuf = nullptr;                 // OHEM: l_p per pixel (-1 = ignored pixel)
    OhemState* st = nullptr;
    unsigned* hist = nullptr;              // the three radix histograms, right behind st
    float tau = 0.f;
    float ce_scale = 1.f;                  // XENT_OHEM_GRAD: the gradient scale is st->gscale * ce_scale (fcn8s_set_lovasz's ce_weight)
    const uint8_t* codes = nullptr;        // fcn8s_op_softmax_xent_px: the distance code of every pixel (indexed like the labels), or nullptr: no pixel weights
    const float* ptab = nullptr;           // ... and the 256 weights b = ptab[code]; XENT_WEIGHTED / XENT_OHEM_GRAD then use w = fl(cw[y] * b)
};
// weighted (ohem_thresh == 0) or OHEM loss over the same blocked / plain logits as launch_softmax_xent; partials then hold sum w l_p, and
// finalize_loss divides by st->kept (OHEM) or by npix (weighted).  No host synchronisation.
void launch_softmax_xent_ex(const float* logits, const uint8_t* labels, float* dlogits, double* partials, long long npix, int C, float grad_scale,
                            hipStream_t s, float* colsum, const PixMap* map, int N, const XentEx& x, float ohem_thresh, long long ohem_min_kept);
// loss_out[0] = sum(partials)/npix + 0.5*rate*regsum[0]; with `den`: sum(partials)/den[0] (0 when den[0] == 0); with `terms`: also
// terms[0] = the cross-entropy term, terms[1] = 0, terms[2] = the L2 term (fcn8s_get_loss_terms)
void launch_finalize_loss(const double* partials, int nparts, long long npix, const float* regsum,
                          float rate, float* loss_out, hipStream_t s, const unsigned long long* den = nullptr, float* terms = nullptr);
// ---- the Lovász-softmax loss (lovasz.hip; fcn8s_set_lovasz, fcn8s_op_lovasz_softmax in include/fcn8s_hip.h) ---------------------
// One scratch of `bytes`: double-buffered keys + payloads [segment][class][pixel] (buffer 0's keys become the [class][pixel] gradient
// plane after the sort), the per-tile digit histograms, foreground counts and loss partials, G, V, the participation scales, the
// backward pass's column-sum partials and the Lovász term.
struct LovaszLayout {
    int nseg = 0, C = 0, tiles = 0; long long L = 0, nsc = 0;
    size_t o_keys[2] = {0, 0}, o_pays[2] = {0, 0}, o_hist = 0, o_tcnt = 0, o_part = 0, o_G = 0, o_V = 0, o_w = 0, o_ncls = 0, o_colpart = 0, o_lov = 0;
    size_t bytes = 0;
};
LovaszLayout lovasz_layout(long long npix, int nseg, int C);
double lovasz_bytes(long long npix, int C, int nmask);        // the algorithmic bytes of the forward + backward stages (profile group "lovasz")
// keys, sort, gradient plane and the loss; x = logits or probabilities in plain [npix, C] or blocked (map) slots; mask_dev = uint8[C] or
// null (every class).  The Lovász term lands in ws + o_lov; class_loss (float[nseg C]) may be null.  With `terms` (the model): terms[1] =
// the term and loss_out[0] = (lce terms[0] + llov terms[1]) + terms[2].
void launch_lovasz_loss(const float* x, int is_logits, const uint8_t* labels, const PixMap* map, int N, long long npix, const LovaszLayout& y,
                        int classes_all, const uint8_t* mask_dev, char* ws, float* class_loss, float* terms, float lce, float llov, float* loss_out,
                        hipStream_t s);
// out (+)= lambda d L_lov / d x (x = logits: the softmax Jacobian applied to the plane's rows; probabilities: the rows themselves); zero
// rows for ignored pixels when !accumulate; colsum (may be null): += the column sums of the contribution, in a fixed order
void launch_lovasz_backward(const float* x, int is_logits, const uint8_t* labels, const PixMap* map, int N, long long npix, const LovaszLayout& y,
                            char* ws, float lambda, int accumulate, float* out, float* colsum, hipStream_t s);
void launch_lovasz_total(float* terms, float lce, float* loss_out, hipStream_t s);   // no Lovász term: loss = lce terms[0] + terms[2], terms[1] = 0
// ---- the soft-target term (soft_targets.hip; fcn8s_set_soft_targets, fcn8s_bind_soft_targets in include/fcn8s_hip.h) ------------------
// One launch behind the cross-entropy (and the Lovász term): dlogits (plain [npix, C] or blocked, map) += lambda (T / npix) (s - q) over the pixels of
// U and the columns < K, then one small kernel: term[0] = L_kd, loss[0] += lambda L_kd, lastbias[c] += the contribution's column sums.  probs: the
// target rows, K floats every row_stride floats, in pixel order.  ws: soft_targets_scratch_bytes() of per-block partials.  C <= 64.
size_t soft_targets_scratch_bytes();
double soft_targets_bytes(long long npix, int C, int K);      // the algorithmic bytes (profile group "soft_targets")
void launch_soft_targets(const float* logits, float* dlogits, const float* probs, const uint8_t* labels, const PixMap* map, int N, long long npix, int C,
                         int K, long long row_stride, float lambda, float temperature, int all_pixels, char* ws, float* loss, float* term,
                         float* lastbias, hipStream_t s);
// ---- the entropy term (entropy_min.hip; fcn8s_set_entropy_term, fcn8s_op_entropy_term in include/fcn8s_hip.h) --------------------------
// One launch behind the soft-target term: dlogits (plain [npix, C] or blocked, map; null: not touched) += coef (-s (ls + h_p)) over the pixels of U
// and the columns < K, then one small kernel: term[0] = L_ent, loss[0] += weight L_ent (null: the op), bias[c] += (bias_add) or = the contribution's
// column sums, c < C (null: none).  ws: entropy_term_scratch_bytes() of per-block partials, 8-byte aligned.  2 <= K <= C <= 64.
size_t entropy_term_scratch_bytes();
double entropy_term_bytes(long long npix, int C);             // the algorithmic bytes (profile group "entropy_term")
void launch_entropy_term(const float* logits, float* dlogits, const uint8_t* labels, const PixMap* map, int N, long long npix, int C, int K, int pixel_set,
                         int first_image, float weight, char* ws, float* loss, float* term, float* bias, int bias_add, hipStream_t s);
// ---- the focal loss (focal.hip; fcn8s_set_focal, fcn8s_op_focal_xent in include/fcn8s_hip.h) ------------------------------------------
// One launch in the cross-entropy's place: dlogits (plain [npix, C] or blocked, map; null: not touched) = the focal gradient rows (stored; zeros for
// ignored pixels and for slots outside the image), then one small kernel: sum_out[0] = the double sum of w_p f l (null: not written; the model hands it
// to finalize_loss as its one partial), loss[0] = fl(sum / npix) (null: the model), st = the loss state that receives |V| (null: none), bias[c] = the
// gradient's column sums, c < C (null: none).  cw = C class weights (null: all 1); codes (indexed like the labels) and ptab (256 weights) both set or
// both null.  ws: focal_xent_scratch_bytes() of per-block partials, 8-byte aligned.  2 <= C <= 64, 0 < gamma <= 8.
size_t focal_xent_scratch_bytes();
double focal_xent_bytes(long long npix, int C, bool codes);   // the algorithmic bytes (profile group "focal_xent")
void launch_focal_xent(const float* logits, float* dlogits, const uint8_t* labels, const float* cw, const uint8_t* codes, const float* ptab, const PixMap* map,
                       int N, long long npix, int C, float gamma, float gscale, char* ws, double* sum_out, float* loss, OhemState* st, float* bias, hipStream_t s);
void launch_softmax_argmax(const float* logits, float* softmax_out, long long* argmax_out,
                           long long npix, int C, hipStream_t s, const PixMap* map = nullptr, int N = 0);
// ---- the k = 2s transposed conv as one GEMM (see PixMap): operand / result re-layouts, all tiny next to the GEMMs -------------
// A[(n,q,qx)][(a,b,ci)] = x[n, q-1+a, qx-1+b, ci] (0 outside), row stride KP >= 4C (columns >= 4C zero)
void launch_tconv_im2col(const float* x, float* A, int N, int Hi, int Wi, int C, int KP, hipStream_t s);
// dx[n,i,j,ci] = sum_{a,b} dA[(n, i+1-a, j+1-b)][(a,b,ci)]
void launch_tconv_col2im(const float* dA, float* dx, int N, int Hi, int Wi, int C, int KP, hipStream_t s);
// w[K,K,Cout,Cin] (K = 2S) -> b2[4C][S*S*C] (forward B operand), b2t[S*S*C][KP] (data-gradient B operand, columns >= 4C zero), bias tiled to S*S*C
void launch_tconv_pack_gemm(const float* w, const float* bias, float* b2, float* b2t, float* bias_tiled, int C, int S, int KP, hipStream_t s);
// dw[K,K,Cout,Cin] += from db2[KP][S*S*C] (rows >= 4C ignored)
void launch_tconv_unpack_dw(const float* db2, float* dw, int C, int S, hipStream_t s);
void launch_unblock_logits(const float* blocked, float* nhwc, const PixMap& map, int N, int C, hipStream_t s);
void launch_onehot_to_ids(const void* oh, int elem_bytes, long long npix, int C, uint8_t* ids, int* bad, hipStream_t s);
void launch_confusion(const uint8_t* labels, const long long* pred, long long npix,
                      unsigned long long* conf, int C, hipStream_t s);
// skinny.hip: 1x1 convs with <= 32 output (forward, weight gradient) or input (data gradient) channels; false = shape not covered
// M rows in `images` images of M / images rows each: whether K is split is decided per image (head_fwd_splits, split_route.h), never by M
bool launch_head_fwd(const float* x, const float* w, const float* bias, float* y, long long M, int images, int K, int C, float alpha, hipStream_t s,
                     float* scratch = nullptr, size_t scratch_floats = 0);      // scratch: lets ONE image with few row blocks split K over more blocks (two-pass sum)
bool launch_head_dgrad(const float* dy, const float* wt, const float* mask, float mask_scale, float* dx, long long M, int K, int C, float alpha,
                       hipStream_t s);
bool launch_head_wgrad(const float* x, const float* dy, float* dw, long long M, int K, int C, float alpha, hipStream_t s);
// bf16_train: max-pool backward (ReLU fused) whose output is the padded bf16 copy of dZ (interior; border zero already) plus db[c] += column sums of dZ
bool launch_maxpool_bwd_bf16(const float* x, const float* dy, unsigned short* dzb, float* db, int N, int H, int W, int C, hipStream_t s, const unsigned char* route = nullptr, long long dzb_ps = 0);
void launch_colsum(const float* x, float* out, long long rows, int C, hipStream_t s);      // out[c] += sum_r x[r,c]
void launch_sumsq(const float* x, float* out, long long n, hipStream_t s);                  // out[0] += sum x^2
void launch_axpy(float* y, const float* x, float a, long long n, hipStream_t s);           // y += a*x
// optim.hip: gradient accumulation over micro-batches, the global-norm clip, the optimizers and the moving average of the parameters
void launch_grad_accumulate(float* dst, const float* src, long long n, int mode, hipStream_t s);   // mode 0: dst = src, 1: dst += src; any float alignment
constexpr int kGradNormBlocks = 2048;                                      // blocks (and partials) of the norm pass: a constant, never the device's CU count
struct UpdateStats { float norm, clip, scale; int ok; unsigned long long skipped; };      // what grad_norm_finalize writes (a model's slab)
// S = sum (double)g^2 through `partials` (kGradNormBlocks doubles) in a fixed order; then {norm, c, s, ok} and, if !ok, ++skipped into `out`.
// as_floats: `out` is float[5] = {norm, c, s, ok (1.0f / 0.0f), 0} instead (fcn8s_op_grad_norm); the word at index 3 is non-zero exactly when ok
void launch_grad_norm(const float* g, long long n, float grad_scale, float max_norm, double* partials, void* out, bool as_floats, hipStream_t s);
// One optimizer step over n floats at any float alignment of any pointer.  opt: FCN8S_OPT_TF_ADAM (p0 .. p3 = lr_t, beta1, beta2, eps; m, v) or
// FCN8S_OPT_SGD_MOMENTUM (p0, p1 = lr, momentum; m is the buffer, v null).  The gradient is scaled by gs, or, when s_dev != nullptr, by *s_dev, and
// then *ok_dev == 0 means that nothing is touched.  shadow != nullptr: the average s <- s - ema_w (s - theta) of the new theta in the same pass,
// w = (float)(1 - decay_t), the same bits as launch_ema_update gives.
struct UpdateArgs {
    int opt; float* theta; const float* g; float* m; float* v; float* shadow; long long n;
    float p0, p1, p2, p3, gs; const float* s_dev; const int* ok_dev; float ema_w;
};
void launch_update(const UpdateArgs& a, hipStream_t s);
// TF-Adam's step size at step t (1-based) with both bias corrections folded in
inline float tf_adam_lr_t(float lr, float b1, float b2, long long t)
{
    return lr * (float)std::sqrt(1.0 - std::pow((double)b2, (double)t)) / (float)(1.0 - std::pow((double)b1, (double)t));
}
// launch_ema_update: the average alone (ok_dev may be null); launch_swap: a <-> b.  Any float alignment of any pointer.
void launch_ema_update(float* sh, const float* theta, long long n, float w, const int* ok_dev, hipStream_t s);
void launch_swap(float* a, float* b, long long n, hipStream_t s);
// weight re-layouts (run once per step, tiny next to the convs)
void launch_flip_transpose(const float* w, float* wt, int taps, int Cin, int Cout, hipStream_t s); // wt[T-1-t][co][ci] = w[t][ci][co]
void launch_pad_cin(const float* w, float* w4, int taps, int Cin, int Cinp, int Cout, hipStream_t s);
void launch_tconv_phase_pack(const float* w, float* wp, int K, int S, int C, hipStream_t s);
void launch_dropout_mask(float* mask, long long n, float keep_prob, unsigned long long seed,
                         unsigned int stream_id, hipStream_t s);
// Winograd F(tile x tile, 3x3) transforms (tile = 2, 4 or 6) around P = (tile+2)^2 batched GEMMs; C % 4 == 0; H, W % tile == 0 for
// tile 2 (tiles 4 and 6 handle partial edge tiles; T = N * ceil(H/tile) * ceil(W/tile)).
// KS = 3: plain 3x3 conv.  KS = 7: the filter is cut into a 3x3 grid of 3x3 sub-filters whose products add up in the
// Winograd domain (GEMM depth 9*C); u / v rows are then [sub][channel].
int wino_r(int KS);                 // sub-filter size: 3 for 3x3 kernels; 7x7 (fc6): 4
int wino_nsub(int KS);              // sub-filters per dimension: ceil(KS / r)
int wino_alpha(int tile, int KS);   // tile + r - 1; the number of Winograd positions is alpha^2
long long wino_slab(long long T, int C);   // floats between the slabs of consecutive Winograd positions of a [P][T][C] tensor (T*C + skew)
void launch_wino_filter(int tile, const float* w, float* u, int Cin, int Cout, int KS, hipStream_t s, int transpose_out = 0, float* u_mfma64 = nullptr);   // w[KS*KS][Cin][Cout] -> u[P][nsub*Cin][Cout]  (transpose_out: u[P][Cout][Cin], KS = 3 only; u_mfma64: F(6x6,3x3) 64 -> 64, a second copy in wino_gemm_out64_kernel's operand order)
// F(6x6,3x3), 64 -> 64 channels, pooled: the 64 position GEMMs, the output transform (bias, ReLU) and the 2x2/2 max-pool with its argmax bytes in one kernel
// (wino_fused64.hip) -- v[64][T][64] and the MFMA-ordered bank straight to pool [N,H/2,W/2,64] and pidx (may be null); M is never written.  false: not launched.
bool launch_wino_gemm_out64(const float* v, const float* u_mfma64, const float* bias, float* pool, unsigned char* pidx, int N, int H, int W, hipStream_t s, int nt = -1);   // nt: 0 / 1 overrides the size rule for the non-temporal instantiation
size_t wino_gemm_out64_bank_floats();      // floats of the MFMA-ordered bank
void launch_wino_input(int tile, const float* x, float* v, int N, int H, int W, int C, int KS, hipStream_t s, unsigned* rbits_out = nullptr);   // x[N,H,W,C] -> v[P][T][nsub*C]
void launch_wino_input_conv1(const float* x0, const float* w4, const float* bias, float* v, int N, int H, int W, hipStream_t s, unsigned* rbits_out = nullptr);   // conv1_1 + conv1_2's F(6x6,3x3) input transform
void launch_wino_input_xb(const float* x, float* v, unsigned short* xb, int N, int H, int W, int C, hipStream_t s, unsigned* rbits_out = nullptr);   // F(6x6,3x3), + padded bf16 copy of x
// F(4x4,3x3) only: V = B^T dy B (input transform of the data-gradient conv) AND dM = A dy A^T (weight-gradient transform) from
// one read of dy; returns false if the shape is not covered.
// pidx != nullptr: `dy` is instead the gradient of the 2x2/2 max-pool output, [N,H/2,W/2,C], and pidx the per-window argmax bytes
// written by launch_wino_output -- the max-pool backward (with the ReLU mask) is applied on the fly and dy never exists in HBM.
bool launch_wino_input_dout(int tile, const float* dy, float* v, float* dm, int N, int H, int W, int C, hipStream_t s, const unsigned char* pidx = nullptr);
void launch_wino_output(int tile, const float* m, const float* bias, const float* addend, const float* mask, float mask_scale,
                        int relu, float* y, int N, int H, int W, int C, int dropout, float keep, unsigned long long seed,
                        unsigned int stream_id, hipStream_t s, float* pool = nullptr, unsigned char* pidx = nullptr, int KS = 3,
                        unsigned* rbits_out = nullptr, const unsigned* rbits_in = nullptr);                      // m[P][T][C] -> y[N,H,W,C]
// rbits_out: also record (y > 0) as one bit per element (wino_rbits_words() words); rbits_in: use such a record instead of `mask`
size_t wino_rbits_words(int tile, int N, int H, int W, int C);
// (pool != nullptr: also writes the 2x2/2 max-pool of y, [N,H/2,W/2,C] -- the tiles are aligned with the pool windows -- and,
//  if pidx != nullptr, one byte per pooled element: index 0..3 of the window's first maximum, 4 if that maximum is not > 0)
void launch_wino_dout(int tile, const float* dy, float* dm, int N, int H, int W, int C, hipStream_t s, int KS = 3, const unsigned char* pidx = nullptr);   // dy -> dm[P][T][C] = A dY A^T  (tile 6 with pidx: dy is d(pool), routed through the argmax bytes)
// F(6x6,3x3) data gradient as the adjoint of the forward algorithm: dv[P][T][C] = dM U^T -> dx = overlap-added B dv B^T (+ skip addend, ReLU mask)
void launch_wino_dgrad_output_dout(const float* dv, const unsigned* rbits_in, float* dm, int N, int H, int W, int C, hipStream_t s);   // ... followed in registers by the previous layer's dM = A dZ A^T (dZ is not written)
void launch_wino_dgrad_output_sub44(const float* dv, float* dx, int N, int H, int W, int C, hipStream_t s);   // fc6: see winograd.hip
void launch_wino_dgrad_output(const float* dv, const float* addend, const float* mask, float mask_scale, const unsigned* rbits_in, float* y,
                              int N, int H, int W, int C, hipStream_t s);
bool launch_wino_out_in(const float* m, const float* bias, float* v, unsigned* rbits_out, int N, int H, int W, int C, hipStream_t s, bool always = false);   // conv L's output transform + conv L+1's input transform in one kernel (Y never written); false = shape not covered
void launch_wino_dfilter(int tile, const float* du, float* dw, int Cin, int Cout, int KS, hipStream_t s);        // du[P][nsub*Cin][Cout] -> dw[KS*KS][Cin][Cout]
// fc6 through 14x14 real-DFT tiles (fft_fc6.hip): 292 real GEMM planes, T = N * ceil(H/8) * ceil(W/8) tiles, slabs wino_slab(T, C) apart
int fft_fc6_planes();
long long fft_fc6_tiles(int N, int H, int W);
void launch_fft_fc6_filter(const float* w, float* uf, int Cin, int Cout, hipStream_t s);                 // w[7][7][Cin][Cout] -> uf[292][Cin][Cout]
void launch_fft_fc6_dfilter(const float* duf, float* dw, int Cin, int Cout, hipStream_t s);              // transpose of the filter transform: duf[292][Cin][Cout] -> dw[7][7][Cin][Cout]
void launch_fft_fc6_input(const float* x, float* xf, int N, int H, int W, int C, hipStream_t s);          // x[N,H,W,C] -> xf[292][T][C]
void launch_fft_fc6_output(const float* yf, const float* bias, float* y, int N, int H, int W, int C, int relu, int dropout, float keep,
                           unsigned long long seed, unsigned int stream_id, hipStream_t s);                 // yf[292][T][C] -> y[N,H,W,C] + epilogue
void launch_fft_fc6_dout(const float* dz, float* dyf, int N, int H, int W, int C, hipStream_t s);         // transpose of the output transform
void launch_fft_fc6_din(const float* dxf, float* patches, float* dx, int N, int H, int W, int C, hipStream_t s);   // transpose of the input transform (patches: T*196*C floats of scratch)
// params: int[4] per image = {y offset, x offset, flip, brightness on/off}; vlut: [N][256] new V per old V (may be nullptr)
void launch_augment_u8(const unsigned char* img, const unsigned char* lab, unsigned char* oimg, unsigned char* olab, const int* params,
                       const unsigned char* vlut, int N, int H, int W, int Ho, int Wo, int void_id, hipStream_t s);
// params: int[4] per image = {resized height, resized width, y offset, x offset}
void launch_resample_u8(const unsigned char* img, const unsigned char* lab, unsigned char* oimg, unsigned char* olab, const int* params,
                        int N, int H, int W, int Ho, int Wo, int void_id, hipStream_t s);
// tta.hip (fcn8s_predict_tta).  Input: image [N,H,W,3] (dtype 0 uint8, 1 float32 -- float only with Hs = H, Ws = W) -> x0 [N,Hp,Wp,4]: cv2
// INTER_LINEAR resize to Hs x Ws (cv_resize.h), mirror if flip, BGR mean subtraction, zeros (the mean colour) outside [0,Hs)x[0,Ws)
void launch_tta_input(const void* img, int dtype, int N, int H, int W, int Hs, int Ws, int Hp, int Wp, int flip, float* out4, hipStream_t s);
// Accumulate: logits of the padded map described by `map` (map.H x map.W pixels; blocked or NHWC) over [0,Hs)x[0,Ws), un-mirrored if flip,
// bilinear (half-pixel) to H x W, softmax; first: acc = p, else acc += p; last: (acc + p) / npasses -> softmax_out [N,H,W,C] and / or
// argmax_out [N,H,W] (acc not written; may be nullptr when first and last)
void launch_tta_accumulate(const float* logits, const PixMap& map, int N, int Hs, int Ws, int flip, int C, int H, int W, float* acc,
                           int first, int last, int npasses, float* softmax_out, long long* argmax_out, hipStream_t s);
// mc_dropout.hip (fcn8s_op_mc_accumulate / fcn8s_predict_mc).  One sample's logits over [0,H)x[0,W) of `map` into the running sums: acc [N,H,W,C] (sum of the
// softmaxes) and ent_acc [N,H,W] (sum of their entropies); `first` stores, `last` writes no accumulator but the outputs that are not null: the mean softmax,
// its argmax, its entropy, the mutual information.  first && last: the accumulators are not touched (and may be null).
void launch_mc_accumulate(const float* logits, const PixMap& map, int N, int H, int W, int C, float* acc, float* ent_acc, int first, int last,
                          int nsamples, float* softmax_out, long long* argmax_out, float* entropy_out, float* mi_out, hipStream_t s);
// crf.hip (fcn8s_op_crf_meanfield / fcn8s_predict_crf).  One mean-field update qin -> qout [N,H,W,C] (qout != qin, qout != prob; the definition is in
// fcn8s_hip.h): messages from qin over the (2 radius + 1)^2 window of the given dilation weighted by the uint8 image img [N,H,W,3], unary log(prob),
// softmax; am (may be nullptr): the argmax of qout.  Defers FCN8S_ERR_SHAPE for a C / radius that crf_shape_supported refuses.
bool crf_shape_supported(int C, int radius);
void launch_crf_meanfield(const float* qin, const float* prob, const unsigned char* img, int N, int H, int W, int C, int radius, int dilation,
                          float w_app, float w_smooth, float theta_alpha, float theta_beta, float theta_gamma, float* qout, long long* am, hipStream_t s);
// am[i] = argmax_c p[i, c], lowest index on ties
void launch_crf_argmax(const float* p, long long npix, int C, long long* am, hipStream_t s);
// cityscapes.hip (fcn8s_op_cityscapes_pair; the definition is in fcn8s_hip.h).  One clear (work, or counts [N][3] when inst == nullptr), the counting kernel
// (conf +=; with inst the per-image tables and error counters in work) and, with inst, the compaction of work into entries [N][max_entries][4] and counts [N][3].
// P < 2^31; work: cityscapes_work_bytes(N) bytes, 16-byte aligned.
size_t cityscapes_work_bytes(int N);
void launch_cityscapes_pair(const uint8_t* gt, const uint16_t* inst, const void* pred, int pred_kind, int N, long long P,
                            unsigned long long* conf, void* work, int* entries, int max_entries, unsigned long long* counts, hipStream_t s);
// reliability.hip (fcn8s_op_reliability_pair; the definition is in fcn8s_hip.h).  One kernel; calib [B][3], sums [4], hist [1 + J][FCN8S_REL_SCORE_BINS][2]
// and bad [2] are accumulated into.  scores / scales: host arrays of J device pointers / floats.  C >= 2, 1 <= B <= 64, 0 <= J <= 3, P < 2^31.
void launch_reliability_pair(const float* prob, const uint8_t* gt, const uint8_t* lut, const float* const* scores, const float* scales, int J,
                             int N, long long P, int C, int B, unsigned long long* calib, unsigned long long* sums, unsigned long long* hist,
                             unsigned long long* bad, hipStream_t s);
// temperature.hip (fcn8s_op_temperature_nll / fcn8s_op_temperature_apply; the definition is in fcn8s_hip.h).  One kernel each.  nll [K], count [1] and
// bad [2] are accumulated into; betas: host array of K floats in [2^-6, 2^6], 1 <= K <= FCN8S_TS_MAX_CANDIDATES.  apply: out (may alias prob) and /
// or entropy_out, not both null.  C >= 2, P < 2^31.
void launch_temperature_nll(const float* prob, const uint8_t* gt, const uint8_t* lut, int N, long long P, int C, const float* betas, int K,
                            unsigned long long* nll, unsigned long long* count, unsigned long long* bad, hipStream_t s);
void launch_temperature_apply(const float* prob, int N, long long P, int C, float beta, float* out, float* entropy_out, hipStream_t s);
// pseudo_label.hip (fcn8s_op_pseudo_label; the definition is in fcn8s_hip.h).  One kernel; hist [C][FCN8S_PL_BINS] (may be null), counts [C][2] and
// misc [3] are accumulated into.  thresholds, out_ids, base, score and labels_out may be null (not labels_out and hist both).  2 <= C <= 255, P < 2^31.
void launch_pseudo_label(const float* prob, int N, long long P, int C, const float* thresholds, const uint8_t* out_ids, int ignore_id,
                         const uint8_t* base, int base_fill, const float* score, float score_max, uint8_t* labels_out,
                         unsigned long long* hist, unsigned long long* counts, unsigned long long* misc, hipStream_t s);
// class_mix.hip (fcn8s_op_class_mix; the definition is in fcn8s_hip.h).  Clear, presence, selection, mix.  2 <= C <= 255, N <= 256, P < 2^31; work:
// class_mix_work_bytes(N) bytes at any alignment; selected_out may be null.
size_t class_mix_work_bytes(int N);
void launch_class_mix(const uint8_t* images, const uint8_t* labels, const int* src, int N, long long P, int C, unsigned long long seed,
                      unsigned long long draw, void* work, uint8_t* out_images, uint8_t* out_labels, uint8_t* selected_out, hipStream_t s);
// strong_augment.hip (fcn8s_op_strong_augment; the definition is in fcn8s_hip.h).  Clear and grey sum (only with a contrast strength), augment.  jitter
// [5], blur [3] and taps [Q][R + 1] are HOST arrays, validated by the caller and passed on by value; any of the first two may be null (taps with blur).
// N <= 256, H * W < 2^31, H, W > R; work: strong_augment_work_bytes(N) bytes at any alignment; params_out may be null.
size_t strong_augment_work_bytes(int N);
void launch_strong_augment(const uint8_t* images, int N, int H, int W, unsigned long long seed, unsigned long long draw, const int* jitter, const int* blur,
                           const unsigned short* taps, void* work, uint8_t* out_images, int* params_out, hipStream_t s);
// fda.hip (fcn8s_op_fda_transfer; the definition is in fcn8s_hip.h).  Tables and pairs, row DFT (MFMA), column DFT, delta, column synthesis, row synthesis
// (MFMA).  N, M <= 256, H * W < 2^31, 0 <= b <= 96, 2 b + 1 <= min(H, W); work: fda_work_bytes(N, M, H, W, b) bytes at any alignment; pair_dev and one of
// the two outputs may be null.
size_t fda_work_bytes(int N, int M, int H, int W, int b);
void launch_fda_transfer(const uint8_t* images, int N, const uint8_t* targets, int M, int H, int W, int b, const int* pair_dev, void* work, uint8_t* out_u8,
                         float* out_f32, hipStream_t s);
// boundary.hip (fcn8s_op_boundary_pair; the definition is in fcn8s_hip.h).  One kernel; rings [R + 1][34][34], bprec / brec [R + 2][34] and bad [1] are
// accumulated into.  1 <= R <= 16, H * W < 2^31.
void launch_boundary_pair(const uint8_t* gt, const void* pred, int pred_kind, int N, int H, int W, int R, unsigned long long* rings,
                          unsigned long long* bprec, unsigned long long* brec, unsigned long long* bad, hipStream_t s);
// boundary_weight.hip (fcn8s_op_boundary_distance; the definition is in fcn8s_hip.h at fcn8s_op_softmax_xent_px).  One kernel; codes [N][H][W] uint8 =
// d2 if <= R * R, else 255.  1 <= R <= 15, H * W < 2^31; any alignment of either pointer.
void launch_boundary_distance(const uint8_t* labels, int N, int H, int W, int R, uint8_t* codes, hipStream_t s);
// regions.hip (fcn8s_op_regions_label / fcn8s_op_regions_clean; the definition is in fcn8s_hip.h).  Both clear the header of `work` first; label writes
// comp and (unless null) area, int32 [N][H][W]; clean rewrites labels in place over `rounds` rounds and writes stats [rounds][4] (may be null).
// H * W < 2^31, N <= 65535, work: regions_work_bytes(N, H, W) bytes, 16-byte aligned.  regions_status: {flag bits, bad pixels} of the last call.
size_t regions_work_bytes(int N, int H, int W);
void launch_regions_label(const void* labels, int label_kind, int N, int H, int W, int connectivity, int* comp, int* area, void* work, hipStream_t s);
void launch_regions_clean(void* labels, int label_kind, int N, int H, int W, int connectivity, const int* min_area, int rounds, void* work,
                          unsigned long long* stats, hipStream_t s);
bool regions_status(const void* work, long long* status2, hipStream_t s);
// panoptic.hip (fcn8s_op_panoptic_pair; the definition is in fcn8s_hip.h).  Clear, count, compact: rows [N][max_rows][3] = {kp, kg, pixels} in no
// particular order, counts [N][4] = {rows found, bad pixels, table too small, pixels counted}.  H * W <= 2^26, N <= 65535, slots a power of two in
// 1 .. 2^28, work: panoptic_work_bytes(N, slots) bytes (0 for slots it refuses), 16-byte aligned.
size_t panoptic_work_bytes(int N, long long slots);
void launch_panoptic_pair(const uint16_t* inst, const void* pred, int pred_kind, const int* comp, int N, int H, int W, void* work, long long slots,
                          long long* rows, long long max_rows, unsigned long long* counts, hipStream_t s);
// instances.hip (fcn8s_op_instance_pair; the definition is in fcn8s_hip.h).  Clear, count, compact: rows [N][max_rows][4] = {kp, v, pixels, sum of
// terms} in no particular order, counts [N][5] = {rows found, labels >= 20, table too small, pixels counted, q out of range}.  inst may be null.
// C >= 20, H * W <= 2^26, N <= 65535, slots a power of two in 1 .. 2^28, work: instance_work_bytes(N, slots) bytes (0 for slots it refuses),
// 16-byte aligned.
size_t instance_work_bytes(int N, long long slots);
void launch_instance_pair(const float* prob, int C, const uint8_t* labels, const int* comp, const uint16_t* inst, int N, int H, int W, void* work,
                          long long slots, long long* rows, long long max_rows, unsigned long long* counts, hipStream_t s);
// wrapping sum over every 61st element's bit pattern (weighted by position): changes whenever an optimizer step or a bulk copy touches the buffer
void launch_fingerprint(const float* x, long long n, unsigned long long* out, hipStream_t s);
void launch_init_normal(float* w, long long n, float stddev, int truncated, unsigned long long seed,
                        unsigned int stream_id, hipStream_t s);

// counter-based RNG shared by the fused dropout epilogue and the mask dump
__host__ __device__ inline uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
__host__ __device__ inline uint32_t philox_u32(unsigned long long idx, unsigned long long seed, uint32_t stream)
{
    uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = stream, c3 = 0x9E3779B9u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
__host__ __device__ inline float philox_uniform(unsigned long long idx, unsigned long long seed, uint32_t stream)
{
    return (float)(philox_u32(idx, seed, stream) >> 8) * (1.0f / 16777216.0f);   // [0,1)
}

}  // namespace fcn8s
