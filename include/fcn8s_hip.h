/* fcn8s_hip.h -- C ABI of libfcn8s_hip.so, the MI355X (gfx950) replacement for
 * the TensorFlow session behind pierluigiferrari/fcn8s_tensorflow's `FCN8s`.
 *
 * The reference has no FFI: its hot path sits behind `tf.Session.run`
 * feed/fetch calls made by class FCN8s (fcn8s_tensorflow.py).  Each entry point
 * below cites the `sess.run` site (or graph-building method) it replaces.
 * Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * Conventions
 *   - all tensors NHWC, C-contiguous; weights in the TensorFlow layouts
 *     (conv HWIO [kh,kw,Cin,Cout]; conv2d_transpose [kh,kw,Cout,Cin]);
 *   - variables are addressed by the reference's variable names
 *     ("conv1_1/filter" ... "fc7_pool4_pool3_conv2d_trans/bias",
 *     fcn8s_tensorflow.py:331-350);
 *   - every function returns FCN8S_OK (0) or an error code; the text is
 *     available from fcn8s_last_error();
 *   - `where` = FCN8S_HOST: pointers are host memory (copied in/out on the
 *     model's stream); FCN8S_DEVICE: pointers are device memory on the model's
 *     GPU and the call is stream-ordered;
 *   - a model is not thread-safe; one model per process per GPU
 *     (the reference is single-threaded, one tf.Session, :65).
 */
#ifndef FCN8S_HIP_H
#define FCN8S_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCN8S_OK            0
#define FCN8S_ERR_BAD_ARG   1   /* facade raises ValueError */
#define FCN8S_ERR_SHAPE     2   /* H or W not a multiple of 32, N<=0 ... (TF: InvalidArgumentError at tf.add :213/:224) */
#define FCN8S_ERR_OOM       3
#define FCN8S_ERR_HIP       4
#define FCN8S_ERR_STATE     5   /* call order violated (e.g. backward before forward) */
#define FCN8S_ERR_NOT_FOUND 6   /* unknown variable / activation name */
#define FCN8S_HOST   0
#define FCN8S_DEVICE 1

#define FCN8S_IMG_U8  0   /* uint8 RGB  [N,H,W,3] */
#define FCN8S_IMG_F32 1   /* float32 RGB [N,H,W,3] */

#define FCN8S_OPT_TF_ADAM      0  /* tf.train.AdamOptimizer, fcn8s_tensorflow.py:256 */
#define FCN8S_OPT_SGD_MOMENTUM 1  /* BASELINE.json config 3 */
#define FCN8S_OPT_NONE         2  /* caller updates the parameter buffer itself (torch optimizer over views) */

#define FCN8S_ERR_RCCL      7   /* a collective of the library's own RCCL communicator failed (fcn8s_comm_*) */
#define FCN8S_MAX_BUCKETS 8       /* upper bound of fcn8s_num_buckets(): gradient buckets in backward-production order */
#define FCN8S_NUM_STAGE_SLOTS 3   /* host-input staging slots (fcn8s_stage_inputs) */

#define FCN8S_PREC_F32     0      /* everything exact fp32 (the reference's arithmetic; default) */
#define FCN8S_PREC_BF16_FC 1      /* BASELINE.json config 5: the forward fc6 / fc7 contractions take bf16-rounded operands on the
                                     bf16 MFMA with fp32 accumulation; everything else, and the whole backward pass, stays fp32 */
#define FCN8S_PREC_F32X3   2      /* fp32-accurate products on the bf16 MFMA: in every LDS-DMA GEMM (Winograd positions, fc6, fc7, the last
                                     transposed conv; forward, data and weight gradients) each fp32 operand is split exactly into three
                                     bf16 pieces and six of the nine piece products are accumulated in fp32 -- error below one fp32
                                     rounding per product, not bit-identical to an fmaf chain; 1.25x faster GEMMs.  Not the default. */

#define FCN8S_PREC_BF16_FWD 3      /* BASELINE.json config 5 taken further ("bf16 fwd / fp32 accum"): besides fc6 / fc7, the forward convolutions of
                                     conv3_1 .. conv5_3 (Cout a multiple of 256) run as direct convolutions with bf16-rounded operands on the bf16
                                     MFMA, fp32 accumulation, fp32 outputs; every other GEMM of the step -- conv1_2 / conv2_x forward, all data and
                                     weight gradients -- uses the F32X3 arithmetic, i.e. all matrix work is on the bf16 MFMA.  Gradients are those of
                                     the fp32 graph evaluated at the bf16-forward activations (straight-through rounding). */
#define FCN8S_PREC_F32X2   4      /* like F32X3 with two pieces per operand, x ~ hi + lo: 16 significand bits of each operand enter the product
                                     (what is cut off is below 2^-17 |x|), three of the four piece products are accumulated in fp32.  Between TF32
                                     (11 bits) and fp32 (24); a reduced-precision mode, half the matrix-pipe and conversion work of F32X3. */
#define FCN8S_PREC_BF16_FWD_X2 5   /* BF16_FWD with the F32X2 arithmetic in place of F32X3 for every GEMM that is not a bf16 forward convolution
                                     (conv1_2 / conv2_x forward, all data and weight gradients): config 5's "bf16 fwd / fp32 accum" with 16-bit
                                     operands in the backward pass */
#define FCN8S_PREC_BF16_TRAIN 6    /* BASELINE.json config 5 with the backward pass on the bf16 pipe as well (round 5): every convolution
                                    * but conv1_1 -- conv1_2 .. conv5_3, fc6, fc7 -- is a DIRECT convolution whose operands are rounded to bf16 (RNE), products and
                                    * sums fp32: forward y = conv(bf16 x, bf16 w); data gradient dx = conv^T(bf16 dy, bf16 w); weight gradient
                                    * dw = corr(bf16 x, bf16 dy); bias gradient, ReLU / dropout masks, pools, the loss, the decoder and the optimizer exact fp32
                                    * on fp32 master weights.  No Winograd transform runs in this mode.  Needs channel widths % 64 == 0. */
#define FCN8S_PREC_FP8_INFER 7     /* INFERENCE ONLY: evaluation, prediction and multi-scale / flip prediction with the convolutions conv1_2 .. conv5_3, fc6 and fc7 on
                                    * the block-scaled MX MFMA with OCP e4m3 operands (E4M3FN: max 448, min subnormal 2^-9, no infinities; not the fnuz format).
                                    *   q(v)  = clamp v to [-448, 448], then round to nearest even e4m3 (on the device and the host; NaN stays NaN);
                                    *   E(a)  = the smallest integer e with a <= 448 2^e, E(0) = 0 (power-of-two scales: every scaling is exact);
                                    *   weights: per layer and output channel co, ew[co] = E(max |W[..., co]|), Wq = q(W 2^-ew[co]);
                                    *   activations: per FP8 layer L, ex[L] = E(amax[L]) from calibration (fcn8s_fp8_calibrate); L's input exists only as a padded
                                    *     e4m3 copy q(x 2^-ex[L]) in 64-channel planes, written by the producer (the previous conv's epilogue inside a block, fc6's for
                                    *     fc7, the byte-max pool on the e4m3 copy of blocks 1, 2 and 5 -- exact: amax(pool) = amax(conv), q is monotone --, a conversion
                                    *     of fp32 conv1_1 / pool3 / pool4);
                                    *   output: y[co] = 2^(ex[L] + ew[co]) sum Xq Wq + b[co], then ReLU; fp32 products and sums.
                                    * conv1_1 (3 input channels), the decoder, softmax / argmax, loss and metrics stay fp32; pool3 / pool4 / fc7 stay fp32 for the skip
                                    * heads.  No split K: an image's logits do not depend on the batch it is predicted in.  Needs channel widths % 64 == 0.  Without a
                                    * calibration an FP8 pass is FCN8S_ERR_STATE; every library call that changes parameters (fcn8s_set_param, fcn8s_init_params, the
                                    * training calls, fcn8s_apply_update, fcn8s_comm_broadcast_params) clears it; writers of ext_params are on their own, as with
                                    * fcn8s_freeze_params.  The calibration survives fcn8s_set_precision.  Training calls in this mode are FCN8S_ERR_STATE.  Frozen models
                                    * quantize each weight bank once; others once per pass.  fcn8s_get_activation(m, "q8:<layer>") returns the dequantized values
                                    * (2^ex code, exact in fp32) of the layer's e4m3 input copy as [N,H,W,Cin]. */
#define FCN8S_FP8_LAYERS 14        /* inputs of conv1_2 .. conv5_3, fc6, fc7, in that order */

typedef struct fcn8s_model fcn8s_model;

typedef struct fcn8s_config {
    int32_t  num_classes;   /* FCN8s(num_classes=...), :19 */
    int32_t  fc6_ksize;     /* 7 (convolutionalized VGG-16 fc6); 0 -> 7 */
    int32_t  widths[7];     /* conv1..conv5, fc6, fc7 channel counts; zeros -> 64,128,256,512,512,4096,4096 */
    int32_t  device_id;     /* HIP device ordinal */
    uint64_t seed;          /* dropout Philox key (per-rank seed for DP) */
    void*    ext_params;    /* optional caller-owned DEVICE buffer of fcn8s_param_floats() floats, or NULL */
    void*    ext_grads;     /* optional caller-owned DEVICE buffer of the same size, or NULL */
} fcn8s_config;

/* ---- layout of the flat variable buffer; pure host logic, needs no GPU ------- */
size_t      fcn8s_param_floats(const fcn8s_config* cfg);             /* size of the flat parameter buffer */
int         fcn8s_layout_num_params(const fcn8s_config* cfg);
int         fcn8s_layout_param(const fcn8s_config* cfg, int index, char name_out[64], int32_t* ndim,
                               int64_t shape[4], int64_t* offset_floats);
int         fcn8s_layout_num_buckets(const fcn8s_config* cfg);       /* = fcn8s_num_buckets of a model made from cfg */
int         fcn8s_layout_bucket(const fcn8s_config* cfg, int bucket, size_t* offset_floats, size_t* nfloats);

/* ---- lifetime: FCN8s.__init__ :19-125 / close :946-952 ------------------- */
int         fcn8s_create(const fcn8s_config* cfg, fcn8s_model** out);
int         fcn8s_destroy(fcn8s_model* m);                           /* frees everything; FCN8S_ERR_RCCL (text: fcn8s_last_error(NULL)) if the model's communicator had failed */
const char* fcn8s_last_error(const fcn8s_model* m);                  /* m may be NULL: last create() error */
/* fcn8s_set_stream: run on the caller's stream (e.g. torch's current stream).  Every later call needs no ordering but that stream's: what it reads
 * must be ready on that stream, and what it writes is ready there when its work on that stream is.  Not all of the work is queued on that stream:
 * the library has streams of its own (staging copies, weight gradients, the communicator), ordered against the caller's by events, and a call
 * that reads a value back copies it with a blocking hipMemcpy after it has synchronised the caller's stream -- right in value, though such a call
 * also waits for whatever the NULL stream is busy with.  The model's internal state (parameters it owns, gradients, workspace, kept filter banks,
 * optimizer slots, the average, metrics) follows the model across streams: when the handle changes, the new stream is made to wait (an event, no
 * host synchronisation) for everything the model has queued on the old one, so a step on stream A followed by a call on stream B is ordered as if
 * both had run on one stream.  The old stream must still exist at that moment; if it does not, or the event fails otherwise, the host is
 * synchronised instead and the model moves all the same.  The caller's own tensors -- images, labels, DEVICE outputs, ext_params / ext_grads when
 * the caller writes them -- remain the caller's to order against the stream it hands over.
 * fcn8s_destroy gives back the per-stream scratch of every stream the model was given. */
int         fcn8s_set_stream(fcn8s_model* m, void* hip_stream);
int         fcn8s_synchronize(fcn8s_model* m);

/* ---- variables (graph.get_tensor_by_name, :331-350; Saver :124,:927,:943) --- */
int    fcn8s_num_params(const fcn8s_model* m);
int    fcn8s_param_info(const fcn8s_model* m, int index, const char** name, int32_t* ndim,
                        int64_t shape[4], int64_t* offset_floats);
int    fcn8s_param_index(const fcn8s_model* m, const char* name);    /* -1 if unknown */
int    fcn8s_set_param(fcn8s_model* m, const char* name, const float* host, size_t nfloats);
int    fcn8s_get_param(fcn8s_model* m, const char* name, float* host, size_t nfloats);
int    fcn8s_get_grad(fcn8s_model* m, const char* name, float* host, size_t nfloats);
void*  fcn8s_param_buffer(fcn8s_model* m, size_t* nfloats);          /* DEVICE pointers, flat, name->offset via param_info */
void*  fcn8s_grad_buffer(fcn8s_model* m, size_t* nfloats);
int    fcn8s_num_buckets(const fcn8s_model* m);                       /* a run-time value (4 today): size nothing by a constant */
int    fcn8s_bucket_range(const fcn8s_model* m, int bucket, size_t* offset_floats, size_t* nfloats);
int    fcn8s_init_params(fcn8s_model* m, uint64_t seed);              /* synthetic init: He-normal VGG, truncated-normal decoder (:159-160) */

/* ---- labels: the reference feeds one-hot rows [N,H,W,C] (placeholder int32 :110, bool from the generator,
 * helpers/ground_truth_conversion_utils.py:84-88).  The kernels consume uint8 class ids; this converts a
 * DEVICE one-hot tensor (elem_bytes 1 = bool/uint8, 4 = int32/float32 bit patterns, non-zero = set) into
 * ids on the device: ids[p] = first c with onehot[p,c] != 0 (= np.argmax of a one-hot row); an all-zero row becomes
 * id 255.  Ids outside [0, C) contribute neither loss nor gradient (softmax_cross_entropy_with_logits of an all-zero
 * row is 0, :253).  `bad_count` (device, may be NULL) is incremented by the number of rows that are not one-hot.       */
int fcn8s_onehot_to_ids(void* stream, const void* onehot_dev, int elem_bytes, int64_t npix, int C,
                        uint8_t* ids_dev, int32_t* bad_count_dev);

/* ---- training: sess.run([train_op,total_loss,global_step]) :554-572 -------- *
 * images: [N,H,W,3]; label_ids: uint8 class ids [N,H,W] (the argmax of the
 * one-hot rows the reference feeds, :110).  loss_out / step_out may be NULL
 * (then the call does not synchronise with the host).                          */
int fcn8s_train_step(fcn8s_model* m, const void* images, int image_dtype, const uint8_t* label_ids,
                     int N, int H, int W, float learning_rate, float keep_prob, float l2_rate,
                     int where, float* loss_out, int64_t* step_out);

/* split-phase form for data-parallel training (no counterpart in the single-device reference): forward + loss, then
 * the backward pass in fcn8s_num_buckets() calls, then the update.  The gradient buffer is cut into that many contiguous buckets in
 * backward-production order -- {fc7, decoder} (68 MB) | {fc6} (411 MB) | {conv4, conv5} (52 MB) | {conv1 .. conv3} (7 MB) at full
 * width -- and bucket b's gradients are final (stream-ordered) once fcn8s_backward_bucket(m, b) has returned, so every bucket's
 * exchange overlaps the rest of the backward pass.  fcn8s_bucket_complete_after(m, b) returns b; it is kept for compatibility.
 * fcn8s_bucket_wait makes another stream (RCCL's, a torch side stream) wait for exactly the last kernel that writes into bucket b
 * -- for fc6 that is its weight gradient, 3 ms of data gradient earlier than the end of call 1 -- without blocking the host; it is
 * valid once call b has returned and until the next fcn8s_forward_loss.
 * `grad_scale` multiplies the gradients inside the update (1/world_size).      */
int fcn8s_forward_loss(fcn8s_model* m, const void* images, int image_dtype, const uint8_t* label_ids,
                       int N, int H, int W, float keep_prob, float l2_rate, int where);
int fcn8s_backward_bucket(fcn8s_model* m, int bucket);
int fcn8s_bucket_complete_after(const fcn8s_model* m, int bucket);
int fcn8s_bucket_wait(fcn8s_model* m, int bucket, void* hip_stream);
int fcn8s_apply_update(fcn8s_model* m, int optimizer, float learning_rate, float grad_scale);   /* waits (stream-ordered) for pending fcn8s_allreduce_bucket calls */
int fcn8s_read_loss(fcn8s_model* m, float* loss_out);                /* synchronises */

/* ---- the training objective: class weights and online hard-example mining (OHEM) -----------------------------------------------
 * The reference trains reduce_mean(softmax_cross_entropy); that stays the default.  Definitions, per rank (a data-parallel run
 * selects on each rank's own batch; there is no cross-rank selection):
 *   P = N*H*W pixels of the batch; V = the valid pixels, label id < C (ids >= C stay "ignore"); l_p = the fp32 per-pixel loss
 *   m + logf(sum exp(v - m)) - v[y_p] (>= 0) exactly as the default kernel computes it; w_c = the class weights (finite, >= 0,
 *   not all zero; default all 1).
 * Weighted (ohem_thresh == 0): L = (1/P) sum_{p in V} w_{y_p} l_p -- denominator P as the reference's reduce_mean, not sum w, so
 *   that data-parallel shards keep matching the big batch under grad_scale = 1/world; dlogits_p = (w_{y_p}/P)(softmax_p - onehot_p).
 *   All weights 1 give the default's loss, dlogits and gradients bit for bit.
 * OHEM (ohem_thresh in (0, 1], a probability as in HRNet): tau = (float)(-log((double)ohem_thresh)); k = min(ohem_min_kept, |V|);
 *   t = min(tau, l_(k)) if k > 0, else tau, with l_(k) the k-th largest l_p over V (multiplicity counts); K = {p in V : l_p >= t}
 *   (ties at t all kept, |K| >= k); L = sum_{p in K} w_{y_p} l_p / |K| (0 when K is empty); dlogits_p = (w_{y_p}/|K|)(softmax_p -
 *   onehot_p) on K, 0 elsewhere.  The selection (a radix select over l_p's float bits) runs on the device: no host round trip.
 * In both modes the L2 term is added as before.  The configuration applies to the training losses only (fcn8s_forward_loss,
 * fcn8s_train_step); fcn8s_eval_step, the metrics and prediction keep the reference's loss.  It survives fcn8s_set_precision and
 * fcn8s_set_option.  Its scratch (state, histograms, OHEM's l_p buffer of P floats) is allocated on first use and counted in
 * "workspace_allocations"; deterministic = 1 keeps OHEM bit-reproducible (integer histograms, per-block loss partials).
 * fcn8s_set_loss: class_weights = host float[nweights], nweights == num_classes, or NULL (all 1); ohem_thresh = 0 (off) or in
 *   (0, 1]; ohem_min_kept >= 0.  NULL weights with ohem_thresh 0 restore the default.  FCN8S_ERR_BAD_ARG for a wrong length,
 *   weights negative / not finite / all zero, a threshold outside {0} U (0, 1] or min_kept < 0.
 * fcn8s_get_loss_stats: |V|, |K| and t of the last training loss (synchronises, like fcn8s_read_loss); in the weighted mode
 *   kept = |V| and threshold = 0.  FCN8S_ERR_STATE when that loss ran without a configuration.                                   */
int fcn8s_set_loss(fcn8s_model* m, const float* class_weights, int nweights, float ohem_thresh, int64_t ohem_min_kept);
int fcn8s_get_loss_stats(fcn8s_model* m, int64_t* valid, int64_t* kept, float* threshold);

/* ---- the training objective: Lovász-softmax (Berman, Rannen Triki, Blaschko, CVPR 2018), a surrogate of the Jaccard index -------------
 * Definitions, per training loss on each rank's own batch (as for OHEM):
 *   P = N*H*W pixels, p = (n*H + h)*W + w, logits z, labels y_p (ids >= C: ignore).  prob[p,k] = expf(z_k - max) / sum in fp32, bit for
 *   bit what fcn8s_op_softmax_argmax and prediction return (same expression, classes summed in order).
 *   Segments s: the whole batch (per_image = 0) or each image (per_image = 1); V_s = the valid pixels of s; |S| = 1 or N.
 *   Participating classes: a mask M over the library's C classes; classes_all = 0 ("present"): C_s = {c : M[c], G_{s,c} > 0};
 *   classes_all = 1: C_s = {c : M[c]}.
 *   Errors: fg = [y_p = c]; e_{p,c} = fl(1 - prob[p,c]) if fg, else prob[p,c] (all in [0, 1]).
 *   Order pi_{s,c} over V_s: e descending, ties by ascending p (= torch.sort(e, descending=True, stable=True)).
 *   Counts at rank r (1-based): f_r = foreground pixels among the first r, G = G_{s,c} = foreground pixels in V_s, I_r = G - f_r,
 *   U_r = G + r - f_r.  Jaccard gradient (exact, cancellation-free; = the reference's J_r - J_{r-1}, J_r = 1 - I_r / U_r, J_0 = 0):
 *   foreground at rank r: g_r = 1 / U_r; background: g_r = I_r / (U_{r-1} U_r), U_0 = G; G = 0: g_1 = 1, every other g_r = 0.
 *   Evaluated in double from the exact integer counts and rounded to float once.
 *   l_{s,c} = sum_r e_{pi(r)} g_r; a segment's loss = the mean of l_{s,c} over C_s (0 when C_s is empty); L_lov = the mean over all
 *   |S| segments (an image without a participating class counts as 0).
 *   L = ce_weight * L_ce + lovasz_weight * L_lov + (the L2 term as before).  L_ce is what fcn8s_set_loss configures (class weights and
 *   OHEM act on the CE term only); (ce_weight, lovasz_weight) = (1, 0) is the default loss bit for bit.
 *   Gradient: d L_lov / d prob[p,c] = g_{rank(p,c)} sgn(prob[p,c] - fg) / (|S| |C_s|) for c in C_s (sgn(0) = 0), 0 elsewhere and on ignored
 *   pixels; dlogits += lovasz_weight * prob (q - <q, prob>) with q the pixel's row of d L_lov / d prob; it reaches the last transposed
 *   conv's bias gradient too.
 * Data parallel: with per_image = 1 and grad_scale = 1/world, equal shards give exactly the big batch's definition (a mean over the
 * images); per_image = 0 sorts each rank's own batch, like OHEM.  The path is deterministic whatever the `deterministic` option says
 * (integer counts, float sums in a fixed order, no float atomics).  The configuration applies to the training losses only
 * (fcn8s_forward_loss, fcn8s_train_step); evaluation, the metrics and prediction keep the reference's loss.  It survives
 * fcn8s_set_precision, fcn8s_set_option and fcn8s_set_loss.  The scratch (double-buffered keys and payloads of |S| x C x P/|S| entries,
 * about 2 x 1.34 GB at 16 x 1024x512 x 20, plus histograms) is grown on first use and counted in "workspace_allocations"; the gradient
 * plane reuses the first key buffer.  Profile group "lovasz".
 * fcn8s_set_lovasz: ce_weight, lovasz_weight finite and >= 0, not both 0; per_image, classes_all in {0, 1}; class_mask = host
 *   uint8[nmask], nmask == num_classes, not all zero (NULL: every class).  (1, 0, ...) restores the default.  FCN8S_ERR_BAD_ARG otherwise.
 * fcn8s_get_loss_terms: the unscaled terms L_ce, L_lov (0 when the Lovász term is off) and the L2 term of the last training loss
 *   (synchronises, like fcn8s_read_loss); FCN8S_ERR_STATE before any training loss.                                                  */
int fcn8s_set_lovasz(fcn8s_model* m, float ce_weight, float lovasz_weight, int per_image, int classes_all, const uint8_t* class_mask, int nmask);
int fcn8s_get_loss_terms(fcn8s_model* m, float* ce, float* lovasz, float* l2);

/* ---- the training objective: boundary-weighted cross-entropy (the definition is at fcn8s_op_softmax_xent_px) ---------------------------
 * The model rule: with the weighting on, every training loss (fcn8s_forward_loss, fcn8s_train_step, each micro-batch of an accumulated
 * update) first computes the distance codes of ITS labels -- those the call was given, one fcn8s_op_boundary_distance launch on the model's
 * stream, profile group "boundary_distance" -- and then runs fcn8s_set_loss's cross-entropy with w_p = fl32(w_{y_p} * table[code(p)]) in
 * place of w_{y_p}: the denominator stays P (|K| under OHEM) and OHEM selects on the unweighted l_p.  Without a configuration of
 * fcn8s_set_loss's the step runs the weighted mode with unit class weights, whatever order the two calls came in, and
 * fcn8s_get_loss_stats reports |V| for it.  A table of all 1.0 changes no bit.  The setting is per model and acts on the training losses
 * only: fcn8s_eval_step, the metrics and prediction keep the reference's loss.  It survives fcn8s_set_precision, fcn8s_set_option,
 * fcn8s_set_loss and fcn8s_set_lovasz; under fcn8s_set_lovasz it acts on the CE term only, like the class weights.  Data parallel: each rank
 * weights its own labels.  The codes ([N, H, W] bytes) are allocated on first use and counted in "workspace_allocations"; while the
 * weighting is off nothing is allocated and no kernel is launched.
 * fcn8s_set_boundary_loss: radius in 1 .. 15 and table256 = 256 host floats, each finite and >= 0; radius 0 with a NULL table switches the
 *   weighting off.  FCN8S_ERR_BAD_ARG for anything else (a table without a radius, a radius without a table, a radius outside 1 .. 15, a
 *   negative or non-finite entry); FCN8S_ERR_STATE for switching it on under FCN8S_PREC_FP8_INFER.  Synchronises the stream before it replaces the table.
 * fcn8s_get_boundary_codes (tests, inspection): the [N, H, W] codes the last training loss computed, to nbytes = N*H*W host bytes
 *   (synchronises).  FCN8S_ERR_STATE if that loss ran without the weighting, FCN8S_ERR_BAD_ARG for another nbytes.                   */
int fcn8s_set_boundary_loss(fcn8s_model* m, int radius, const float* table256);
int fcn8s_get_boundary_codes(fcn8s_model* m, uint8_t* codes_out, int64_t nbytes);

/* ---- the training objective: soft targets (distillation; Hinton, Vinyals, Dean 2015): KL(teacher || student) at a temperature ---------------
 * Definitions, per training loss on each rank's own batch:
 *   P = N*H*W pixels, p = (n*H + h)*W + w, logits z (the library's C classes), labels y_p.  Bound targets t[p, 0..K), K = ncols <= C (the caller's
 *   logical classes), row p at probs_dev + p * row_stride.  Columns >= K do not take part: target 0, gradient 0 (a padding class's -1e30 logit never
 *   meets a logarithm).  beta = 1 / T, T finite and > 0.  U = the pixels with y_p < C (all_pixels = 0), or every pixel (all_pixels = 1).
 *   For p in U, in fp32 with expf and logf, classes summed in order, no product contracted into a sum:
 *     teacher (the tempered map of temperature.py / fcn8s_op_temperature_apply):
 *       l_c = logf(max(t_c, FLT_MIN)); a_c = beta (l_c - max_c l); Sq = sum_c expf(a_c); q_c = expf(a_c) / Sq; log q_c = a_c - logf(Sq)
 *     student:
 *       b_c = beta (z_c - max_{c<K} z); Ss = sum_c expf(b_c); s_c = expf(b_c) / Ss; log s_c = b_c - logf(Ss)
 *     kd_p = sum_{c<K} q_c (log q_c - log s_c)
 *   L_kd = (T^2 / P) sum_{p in U} kd_p -- the denominator is P, as the cross-entropy's, so equal data-parallel shards keep matching the big batch;
 *   the kd_p are summed in double (per thread, then per block, then over the blocks in a fixed order) and the product is rounded to float once.
 *   L = ce_weight * L_ce + lovasz_weight * L_lov + weight * L_kd + (the L2 term as before).
 *   Gradient: dlogits[p,c] += fl(weight * fl(T / P)) * (s_c - q_c) for p in U and c < K; the same contribution reaches the last transposed conv's
 *   bias gradient.  Class weights, OHEM and the boundary table act on the CE term only.
 *   A target row with a non-finite entry makes that pixel's term and its gradient row NaN, as fcn8s_op_temperature_apply does: the loss shows it and
 *   the guard of fcn8s_set_grad_clip skips the update.
 * One launch behind the cross-entropy (and the Lovász term) plus a one-block reduction, both in front of the loss copy; it works on the logits where
 * they lie (plain or in the blocked layout of "tconv_gemm").  Deterministic whatever the `deterministic` option says: per-block partial sums reduced
 * in a fixed order, no float atomics.  The term acts on the training losses only (fcn8s_forward_loss, fcn8s_train_step, each micro-batch of an
 * accumulated update); evaluation, the metrics and prediction keep the reference's loss and neither consume nor read a binding.  The per-block
 * partials (about 270 KB) are allocated on first use and counted in "workspace_allocations".  Profile group "soft_targets".
 * fcn8s_set_soft_targets: weight 0 switches the term off and drops any binding -- then nothing is launched or allocated and the step is bit for bit
 *   what it was.  FCN8S_ERR_BAD_ARG for a non-finite or negative weight, a temperature that is not finite and > 0, all_pixels outside {0, 1};
 *   FCN8S_ERR_STATE for switching it on under FCN8S_PREC_FP8_INFER.  The setting survives fcn8s_set_precision, fcn8s_set_option, fcn8s_set_loss,
 *   fcn8s_set_lovasz and fcn8s_set_boundary_loss.
 * fcn8s_bind_soft_targets: probs_dev = device float32, N*H*W rows of ncols floats every row_stride floats.  The binding is consumed by exactly one
 *   training loss, which reads the buffer on the model's stream (ordering against the writer is the caller's, as for device images; the buffer must
 *   live until that loss has run).  With the term on and nothing bound a training loss returns FCN8S_ERR_STATE, with a binding for another N, H, W
 *   FCN8S_ERR_SHAPE, both before anything is launched.  FCN8S_ERR_BAD_ARG: NULL or misaligned probs_dev, ncols outside 1 .. num_classes,
 *   row_stride < ncols; FCN8S_ERR_SHAPE: N, H or W <= 0; FCN8S_ERR_STATE: the term is off.
 * fcn8s_get_soft_target_term: the unscaled L_kd of the last training loss (synchronises, like fcn8s_get_loss_terms); FCN8S_ERR_STATE if that loss
 *   ran without the term, or after the term was switched off.  fcn8s_get_loss_terms is what it was.                                       */
int fcn8s_set_soft_targets(fcn8s_model* m, float weight, float temperature, int all_pixels);
int fcn8s_bind_soft_targets(fcn8s_model* m, const float* probs_dev, int N, int H, int W, int ncols, int64_t row_stride);
int fcn8s_get_soft_target_term(fcn8s_model* m, float* kd);   /* unscaled L_kd of the last training loss; synchronises like fcn8s_get_loss_terms */

/* ---- the training objective: an entropy term on the student's own prediction (entropy minimisation: Grandvalet & Bengio 2005; "MinEnt" of ADVENT,
 * Vu et al. 2019; with a negative weight the confidence penalty of Pereyra et al. 2017) -------------------------------------------------------------
 * Definitions, per training loss on each rank's own batch:
 *   P = N*H*W pixels, p = (n*H + h)*W + w, logits z (the library's C classes), labels y_p.  K = ncols, 2 <= K <= C (the caller's logical classes).
 *   Columns >= K do not take part: gradient exactly 0, and a padding class's -1e30 logit never meets expf or a product.  f = first_image >= 0.
 *   U = the pixels of the images n >= f with  y_p >= C (pixel_set = FCN8S_ENT_UNLABELED),  y_p < C (FCN8S_ENT_VALID),  any label (FCN8S_ENT_ALL);
 *   f >= N: U is empty, the term is 0 and nothing changes.
 *   For p in U, in fp32 with expf and logf, classes summed in order, no product contracted into a sum:
 *     b_c = z_c - max_{c<K} z;  S = sum_{c<K} expf(b_c);  s_c = expf(b_c) / S;  ls_c = b_c - logf(S)
 *     h_p = -sum_{c<K} s_c ls_c        (the log-softmax form: an s_c that underflowed multiplies a finite ls_c, so no clamp is needed -- this is
 *                                       not the clamped entropy of the prediction routes)
 *   L_ent = (1 / (P log K)) sum_{p in U} h_p -- the denominator is P, as the cross-entropy's and L_kd's, so equal data-parallel shards keep matching
 *   the big batch; the division by log K puts a pixel's value in [0, 1].  The h_p are summed in double (per thread, then per block, then over the
 *   blocks in a fixed order), the sum is divided by the double P * log((double)K) and the quotient is rounded to float once.
 *   L = (everything as before) + fl(weight * L_ent).
 *   Gradient: dlogits[p,c] += coef * (-(s_c * (ls_c + h_p))) for p in U and c < K, with coef = weight / (P log K) computed in double from the float
 *   weight and rounded to float once.  The sum ls_c + h_p is evaluated with its two logf(S) cancelled on paper: ls_c + h_p = b_c - m_p,
 *   m_p = sum_{c<K} s_c b_c (fp32, classes in order, no product contracted; equal when sum_c s_c = 1), so the kernel computes
 *   coef * (-(s_c * (b_c - m_p))).  Taken as written, fl(ls_c + h_p) on a row of equal logits is what K roundings of sum s_c ls_c leave of
 *   logf(K) - logf(K), a few 1e-7 and not 0; in this form such a row has b = 0, m_p = 0 and a gradient row of exact zeros, and the difference
 *   between the two forms is s_c logf(S) (sum s - 1), below the rounding of either.  h_p and L_ent are the sums written above; the same contribution reaches the last transposed conv's bias gradient.  Every other entry of dlogits gets
 *   -0.0f added, which changes no float.  Class weights, OHEM, the boundary table, the Lovász term and the soft-target term act as before.
 *   A row with a NaN or an infinite logit among its columns < K makes that pixel's h_p and its gradient row NaN: the loss shows it and the guard of
 *   fcn8s_set_grad_clip skips the update.
 * One launch behind the cross-entropy (and the Lovász and soft-target terms) plus a one-block reduction, both in front of the loss copy; it works on
 * the logits where they lie (plain or in the blocked layout of "tconv_gemm").  Deterministic whatever the `deterministic` option says: per-block
 * partial sums reduced in a fixed order, no float atomics.  The term acts on the training losses only (fcn8s_forward_loss, fcn8s_train_step, each
 * micro-batch of an accumulated update); evaluation, the metrics and prediction keep the reference's loss.  The per-block partials (about 270 KB)
 * are allocated on first use and counted in "workspace_allocations".  Profile group "entropy_term", (12 C + 1) bytes per pixel.
 * fcn8s_set_entropy_term: host state only (no launch, no allocation, no synchronisation).  weight: any finite float; > 0 minimises the entropy, < 0
 *   is the confidence penalty, 0 switches the term off -- then nothing is launched or allocated and the step is bit for bit what it was.
 *   FCN8S_ERR_BAD_ARG for a non-finite weight, pixel_set outside {0, 1, 2}, ncols outside 2 .. num_classes, first_image < 0 (whatever the weight);
 *   FCN8S_ERR_STATE for switching it on under FCN8S_PREC_FP8_INFER.  The setting survives fcn8s_set_precision, fcn8s_set_option, fcn8s_set_loss,
 *   fcn8s_set_lovasz, fcn8s_set_boundary_loss and fcn8s_set_soft_targets.
 * fcn8s_get_entropy_term: the unscaled L_ent of the last training loss (synchronises, like fcn8s_get_loss_terms); FCN8S_ERR_STATE if that loss ran
 *   without the term, or after the term was switched off.  fcn8s_get_loss_terms and fcn8s_get_soft_target_term are what they were.
 * fcn8s_op_entropy_term: the same kernel and reduction on the caller's buffers, stream-ordered, allocating nothing: logits and dlogits device float32
 *   [N*HW, C] in the plain layout at any 4-byte alignment, labels device uint8 [N*HW] at any alignment, work = fcn8s_op_entropy_term_work_bytes()
 *   bytes of device scratch at any alignment (work_bytes = what is passed).  term_out[0] = L_ent; bias_out (may be NULL) = the C column sums of the
 *   contribution; dlogits (may be NULL: the term and the column sums only) += the contribution.  FCN8S_ERR_BAD_ARG: a NULL logits, labels, work or
 *   term_out, a misaligned float pointer, a non-finite weight, pixel_set, ncols or first_image as above, C outside 2 .. 64, work_bytes too small;
 *   FCN8S_ERR_SHAPE: N or HW <= 0.  A refused call leaves every output untouched.                                                             */
#define FCN8S_ENT_UNLABELED 0
#define FCN8S_ENT_VALID 1
#define FCN8S_ENT_ALL 2
int fcn8s_set_entropy_term(fcn8s_model* m, float weight, int pixel_set, int ncols, int first_image);
int fcn8s_get_entropy_term(fcn8s_model* m, float* term);     /* unscaled L_ent of the last training loss; synchronises like fcn8s_get_loss_terms */
size_t fcn8s_op_entropy_term_work_bytes(void);
int fcn8s_op_entropy_term(void* stream, const float* logits, float* dlogits, const uint8_t* labels, int N, int64_t HW, int C, int ncols, int pixel_set,
                          int first_image, float weight, void* work, size_t work_bytes, float* term_out, float* bias_out);

/* ---- the training objective: the focal loss (Lin, Goyal, Girshick, He, Dollár, ICCV 2017), the smooth counterpart of OHEM -----------------------------
 * Definitions, per training loss on each rank's own batch:
 *   P = N*H*W pixels, logits z over the library's C columns, labels y_p (ids >= C: ignored, no loss and a gradient row of zeros).  gamma: a float with
 *   0 < gamma <= 8 (0: off).  w_p = w_{y_p}, the class weight of fcn8s_set_loss (1 without one); under fcn8s_set_boundary_loss w_p = fl(w_{y_p} *
 *   table[code(p)]), exactly as the weighted mode forms it.  Class weights so act as the alpha of the alpha-balanced focal loss.
 *   Per valid pixel, in fp32 with expf and logf, classes summed in order, no product contracted into a sum:
 *     m = max_c z_c;  e_c = expf(z_c - m);  S = sum_c e_c;  l = (m + logf(S)) - z_y            (the cross-entropy's own l_p, >= 0)
 *     R = sum_{c != y} e_c (class order, y skipped);  u = R / S (= 1 - s_y, with no subtraction);  s_y = e_y / S
 *     u == 0:  f = 0, a = 0
 *     else:    t = expf((gamma - 1) * logf(max(u, FLT_MIN)));  f = t * u;  a = t * (u + gamma * (l * s_y))
 *   L_foc = (1/P) sum_{p valid} w_p (f l): the float product f l times the float w_p, multiplied and summed in double (per thread, then per block, then
 *   over the blocks in a fixed order); the sum is divided by P and rounded to float once.  The denominator is P, as the cross-entropy's, so equal
 *   data-parallel shards keep matching the big batch.
 *   Gradient: d(u^gamma l)/dz_c = (s_c - [c = y]) (u^gamma + gamma l s_y u^(gamma - 1)), so a is the scalar that multiplies the cross-entropy's
 *   gradient row.  g_p = gscale * w_p (gscale = ce_weight / P as the cross-entropy forms it);  c_p = g_p * a;
 *     dlogits[p,c] = e_c * (c_p / S) for c != y;   dlogits[p,y] = -(c_p * u)                   (the y column never comes from s_y - 1)
 *   A padding column's -1e30 logit gives e = 0 and a gradient of exactly 0.  gamma = 1 gives t = 1 exactly.  Non-finite logits behave as in the
 *   cross-entropy.
 *   L = ce_weight * L_foc + (the Lovász, soft-target, entropy and L2 terms as before): L_foc stands in L_ce's place, in the `ce` slot of
 *   fcn8s_get_loss_terms too; fcn8s_get_loss_stats reports |V|, kept = |V| and threshold 0, with or without a configuration of fcn8s_set_loss's.
 * OHEM together with gamma > 0 is refused, because both address the same thing: fcn8s_set_focal returns FCN8S_ERR_STATE while an OHEM threshold is
 * set, and fcn8s_set_loss returns it for an OHEM threshold while gamma > 0.
 * One launch in the cross-entropy's place plus a one-block reduction; it works on the logits where they lie (plain or in the blocked layout of
 * "tconv_gemm") and moves the bytes of the weighted cross-entropy.  Deterministic whatever the `deterministic` option says: per-block partial sums
 * reduced in a fixed order, no float atomics.  The setting acts on the training losses only (fcn8s_forward_loss, fcn8s_train_step, each micro-batch of
 * an accumulated update); evaluation, the metrics and prediction keep the reference's loss.  The per-block partials (about 280 KB) and, without a
 * configuration of fcn8s_set_loss's, the loss state that holds |V| are allocated on first use and counted in "workspace_allocations".  Profile group
 * "focal_xent" (in place of "softmax_xent"), (8 C + 1) bytes per pixel, + 1 with the boundary codes.
 * fcn8s_set_focal: host state only (no launch, no allocation, no synchronisation).  gamma 0 switches it off -- then nothing new is launched or
 *   allocated and the step is bit for bit what it was.  FCN8S_ERR_BAD_ARG for a non-finite gamma, gamma < 0 or gamma > 8; FCN8S_ERR_STATE for
 *   switching it on under FCN8S_PREC_FP8_INFER or while OHEM is configured.  The setting survives fcn8s_set_precision, fcn8s_set_option and the
 *   other loss setters.
 * fcn8s_op_focal_xent: the same kernel and reduction on the caller's buffers, stream-ordered, allocating nothing: logits device float32 [npix, C] in
 *   the plain layout at any 4-byte alignment, labels (and codes) device uint8 [npix] at any alignment, class_weights_dev = C device floats or NULL (all
 *   1), codes_dev and table256_dev (256 device floats) both set or both NULL, work = fcn8s_op_focal_xent_work_bytes() bytes of device scratch at any
 *   alignment (work_bytes = what is passed), gscale = 1 / (float)npix.  dlogits (may be NULL) is STORED, not added to: this is the cross-entropy's
 *   role.  loss_dev[0] = L_foc; bias_out (may be NULL) = the C column sums of dlogits.  FCN8S_ERR_BAD_ARG: a NULL logits, labels, loss_dev or work, a
 *   misaligned float pointer, gamma not in (0, 8] (gamma = 0 is what the plain ops compute), C outside 2 .. 64, codes without a table or a table
 *   without codes, work_bytes too small; FCN8S_ERR_SHAPE: npix <= 0.  A refused call leaves every output untouched.                            */
int fcn8s_set_focal(fcn8s_model* m, float gamma);
size_t fcn8s_op_focal_xent_work_bytes(void);
int fcn8s_op_focal_xent(void* stream, const float* logits, const uint8_t* labels, const float* class_weights_dev, const uint8_t* codes_dev,
                        const float* table256_dev, float gamma, float* dlogits, float* loss_dev, float* bias_out, int64_t npix, int C, void* work,
                        size_t work_bytes);

/* ---- the update: gradient accumulation over micro-batches, a global-norm clip and a non-finite guard (not in the reference, whose step is
 * one batch, one tf.train.AdamOptimizer.minimize, fcn8s_tensorflow.py:256) ------------------------------------------------------------------
 * Accumulation.  The model owns one accumulator acc of fcn8s_param_floats() floats, cut into the gradient buffer's buckets; it is allocated at
 *   the first fold (one "workspace_allocation") and kept until fcn8s_destroy.  Bucket b has a pending count k_b >= 0.  After
 *   fcn8s_backward_bucket(m, b) the caller makes ONE of two calls:
 *     fold  (flush = 0; a micro-batch that is not the last): acc[b] = g[b] if k_b == 0, else acc[b] = acc[b] + g[b]; k_b += 1; g[b] untouched;
 *     flush (flush = 1; the last micro-batch): g[b] = g[b] + acc[b]; k_b = 0.  With k_b == 0 it launches nothing.  The bucket's event is
 *       recorded again behind the flush kernel, so fcn8s_bucket_wait and fcn8s_allreduce_bucket still wait for the last kernel that writes
 *       the bucket: a data-parallel run exchanges once per update, on the last micro-batch, with the overlap it has without accumulation.
 *   One fp32 add per element and call: after A micro-batches g = fl(fl(g1 + g2) + g3) ..., what NumPy float32 gives bit for bit.
 *   Nothing is divided by A here: the caller passes grad_scale = 1 / (A * world) to the update as it passes 1 / world without accumulation.
 *   The L2 term is in every micro-batch's g (A of them times 1/A: the big batch's).  For the default and the class-weighted loss (both with
 *   denominator P) A micro-batches of n images at keep_prob = 1 are the batch of A n images up to fp32 summation order; OHEM and Lovász
 *   select per micro-batch, as they select per rank.  Micro-batches may differ in shape and precision mode (the gradients are
 *   parameter-sized fp32).  Profile group "grad_accumulate" (12 bytes per element and call, 8 for a first fold).
 *   FCN8S_ERR_STATE: bucket b's fcn8s_backward_bucket has not run since the last fcn8s_forward_loss; a second fold / flush of b for the same
 *   backward pass; the bucket is being all-reduced; fcn8s_apply_update while any k_b > 0 (parameters and step untouched: a forgotten flush
 *   never loses gradients silently).  fcn8s_train_step flushes every bucket behind its backward call and divides its scale by (pending + 1).
 * Clipping and the guard.  max_norm in (0, +inf], 0 = off (default).  When it is on, fcn8s_apply_update first computes on the device
 *     S = sum_i (double)g_i^2 over the whole flat buffer, in a fixed order whatever "deterministic" says and on every device: 2048 blocks of
 *         256 lanes; a lane adds the squares of its elements (in ascending index, stride 2048 * 256 float4) in double; lanes are summed per wave
 *         by a shuffle tree, waves in index order; the 2048 block sums go to a slab, of which one block's lane t adds entries 8t .. 8t + 7 in
 *         index order before the same tree.  No float atomics: two runs give the same bits.
 *     norm = (float)(|grad_scale| * sqrt(S));   c = max_norm / fmaxf(norm, max_norm) in fp32 (tf.clip_by_global_norm; c = 1 for +inf);
 *     s = grad_scale * c in fp32;               ok = isfinite(norm).
 *   The optimizer kernel reads s and ok from device memory: gr = g * s where it computes g * grad_scale otherwise; if !ok it touches neither
 *   the parameters nor the optimizer's slots and a device counter `skipped` goes up by one.  The global step (a host counter) advances either
 *   way and the step does not synchronise.  max_norm = +inf therefore means "guard only".  norm <= max_norm gives s == grad_scale bit for
 *   bit.  The norm is taken after the all-reduce: every replica computes the same s.  Profile group "grad_norm" (4 bytes per element).
 *   The setting survives fcn8s_set_precision, fcn8s_set_option and freezing.  fcn8s_set_grad_clip: NaN or negative is FCN8S_ERR_BAD_ARG.
 *   fcn8s_get_update_stats: norm, c, s of the last update and the updates skipped so far (synchronises); any pointer may be NULL;
 *   FCN8S_ERR_STATE if the last update ran without a clip setting.  Under FCN8S_PREC_FP8_INFER fcn8s_accumulate_bucket refuses like the
 *   other training calls.                                                                                                                  */
int fcn8s_accumulate_bucket(fcn8s_model* m, int bucket, int flush);   /* after fcn8s_backward_bucket(m, bucket): 0 = fold, 1 = flush */
int fcn8s_accumulate_pending(const fcn8s_model* m);                   /* micro-batches folded and not yet flushed (max over buckets) */
int fcn8s_accumulate_discard(fcn8s_model* m);                         /* k_b = 0 for every b; keeps the memory */
int fcn8s_set_grad_clip(fcn8s_model* m, float max_norm);
int fcn8s_get_update_stats(fcn8s_model* m, float* norm, float* clip_coef, float* scale, int64_t* skipped);

/* ---- the average: an exponential moving average of the parameters, kept on the device (not in fcn8s_tensorflow.py; what
 * tf.train.ExponentialMovingAverage(decay, num_updates=global_step) gives a TensorFlow 1.x training script) -----------------------------------
 * Shadow.  The model owns one shadow s of fcn8s_param_floats() floats.  It is allocated when the average is first switched on (fcn8s_set_ema
 *   with decay > 0, or fcn8s_set_ema_state), counted as one "workspace_allocation", and kept until fcn8s_destroy.  At that moment s = theta
 *   (a stream-ordered device copy).  decay = 0 switches the average off and keeps the memory and the contents; switching it on again continues
 *   from them.  fcn8s_ema_reset sets s = theta.  With the average never switched on nothing is allocated and no kernel below runs.
 * Update.  After every applied update, with t the new global step (what fcn8s_global_step returns after the call):
 *     d_t = warmup ? min(d, (1 + t) / (10 + t)) : d   in double (TensorFlow's num_updates rule);   w = (float)(1.0 - d_t);
 *     s_i <- s_i - w (s_i - theta_i)   in fp32, theta the parameters after the update: d = fl(s_i - theta_i), then one fused multiply-add
 *     fma(-w, d, s_i) (assign_moving_average without zero-debias).  d in (0, 1); 0 = off.
 *   TF-Adam and SGD-momentum compute theta and their slots with the expressions (and the bits) of the kernels that run without an average and
 *   fold the new theta into s in the same pass: 36 / 28 bytes per element instead of 28 / 20 (profile groups "adam" / "sgd_momentum").  With
 *   FCN8S_OPT_NONE the caller has written theta; fcn8s_apply_update folds theta as it stands on the stream into s (group "ema_update", 12 bytes
 *   per element).  fcn8s_train_step follows through its fcn8s_apply_update.
 * Guard.  An update that the non-finite guard skips (ok == 0) leaves s untouched, as it leaves theta and the slots; the step still advances.
 * Accumulation.  fcn8s_accumulate_bucket never touches s; only the update does.
 * Data parallel.  Replicas hold identical theta, hence identical s: nothing is exchanged.
 * Swap.  fcn8s_ema_swap exchanges theta and s in place (one kernel, no third buffer; group "ema_swap", 16 bytes per element) and toggles a
 *   `swapped` flag.  The live parameters changed: like fcn8s_set_param it leaves the frozen state, drops the cached banks and clears an fp8
 *   calibration.  While swapped, everything that reads parameters (evaluation, every prediction call, fp8 calibration, fcn8s_get_param) works on
 *   the averaged weights, fcn8s_get_ema reads the raw ones, and fcn8s_apply_update, fcn8s_train_step, fcn8s_accumulate_bucket, fcn8s_ema_reset
 *   and fcn8s_set_ema_state return FCN8S_ERR_STATE with theta, s, the slots and the step untouched: nobody trains the average by accident.  A
 *   second swap restores the raw weights bit for bit.
 * fcn8s_set_ema: decay NaN, negative or >= 1 is FCN8S_ERR_BAD_ARG; accepted under FCN8S_PREC_FP8_INFER (the training calls refuse there anyway).
 * fcn8s_ema_reset, fcn8s_ema_swap, fcn8s_get_ema without a shadow: FCN8S_ERR_STATE.  fcn8s_get_ema / fcn8s_set_ema_state: the flat shadow, n ==
 *   fcn8s_param_floats() (the layout of fcn8s_get_opt_state); set allocates the shadow if there is none and does not switch the average on.
 * fcn8s_get_ema_info: any pointer may be NULL.  The setting and the shadow survive fcn8s_set_precision, fcn8s_set_option and freezing.       */
int fcn8s_set_ema(fcn8s_model* m, double decay, int warmup);
int fcn8s_ema_reset(fcn8s_model* m);
int fcn8s_ema_swap(fcn8s_model* m);
int fcn8s_get_ema_info(const fcn8s_model* m, double* decay, int* warmup, int* has_shadow, int* swapped);
int fcn8s_get_ema(fcn8s_model* m, float* host, size_t nfloats);
int fcn8s_set_ema_state(fcn8s_model* m, const float* host, size_t nfloats);

/* ---- data parallelism inside the library: one RCCL rank per model (SURVEY section 7 step 7, 8b "RCCL error"; the reference is one
 * tf.Session on one device, fcn8s_tensorflow.py:65, so there is nothing to cite for the collective itself).  A caller that keeps the
 * reference's Python and binds this ABI gets multi-GPU training without torch.distributed:
 *     rank 0: fcn8s_comm_unique_id(id)  -> hand the FCN8S_COMM_ID_BYTES bytes to every rank by any means (file, socket, MPI)
 *     all   : fcn8s_comm_init(m, id, FCN8S_COMM_ID_BYTES, rank, world);  fcn8s_comm_broadcast_params(m, 0)
 *     step  : fcn8s_forward_loss; for b in 0 .. fcn8s_num_buckets-1 { fcn8s_backward_bucket(m, b); fcn8s_allreduce_bucket(m, b) };
 *             fcn8s_apply_update(m, opt, lr, 1.0f / world)
 *     eval  : fcn8s_eval_step ...; fcn8s_comm_allreduce_metrics(m); fcn8s_metrics_get
 * fcn8s_allreduce_bucket queues an in-place SUM all-reduce of the bucket on a stream the library owns, behind the event of the last
 * kernel that writes into the bucket (never behind later backward kernels) and returns at once; fcn8s_comm_wait makes the model's
 * stream wait for all of them (fcn8s_apply_update does it implicitly, and so do fcn8s_get_grad and the next fcn8s_backward_bucket(m, 0);
 * a caller that reads fcn8s_grad_buffer() itself calls fcn8s_comm_wait first).  fcn8s_train_step on a model whose communicator has more
 * than one rank runs exactly this sequence (it never trains diverging replicas silently).  librccl is opened with dlopen at the first
 * fcn8s_comm_* call (no RCCL headers are needed to build the library; environment variable FCN8S_RCCL_LIBRARY names the file to open
 * instead of the soname -- a site's own RCCL build, or the shared-memory stand-in of tests/fake_rccl -- and fcn8s_comm_init refuses a
 * library whose ncclGetVersion is not 2.x, the ABI whose enum values this library declares for itself): a failure there, or at the
 * enqueue of any collective, is FCN8S_ERR_RCCL with RCCL's text in fcn8s_last_error.  Failures AFTER the enqueue -- a peer that dies or
 * hangs -- are caught by a watchdog thread every communicator of more than one rank owns: it polls ncclCommGetAsyncError and the age of
 * EVERY collective in flight (the bucket all-reduces, the parameter broadcast, the metrics all-reduce; each is enqueued under the mutex
 * the watchdog aborts under), and on an asynchronous error, or when a collective has not completed within option "comm_timeout_ms"
 * (default 600 000), calls ncclCommAbort -- RCCL's kernels then leave the streams, so neither the model's stream nor a host
 * synchronisation waits for that peer forever -- and fcn8s_allreduce_bucket / fcn8s_comm_wait / fcn8s_apply_update / fcn8s_comm_* return
 * FCN8S_ERR_RCCL with the reason.  With more than one rank fcn8s_apply_update waits ON THE HOST (polling) for the pending all-reduces
 * before it queues the update: gradients whose exchange was aborted are never applied, and the failure is reported by the very call
 * that would have used them (cost: the host's run-ahead over one kernel launch per step).  fcn8s_comm_allreduce_metrics waits for its
 * sums the same way.  fcn8s_comm_destroy (also run by fcn8s_destroy, before anything else) drains the communicator's stream by polling
 * under the same rules, never by an unconditional synchronisation, and returns FCN8S_ERR_RCCL once if the communicator had failed.      */
/* "dddd:bb:dd.f" of a HIP device (hipDeviceGetPCIBusId): lets a launcher bind each rank's host threads and decode workers to the
 * NUMA node of its GPU through /sys/bus/pci/devices/<id>/local_cpulist (fcn8s_tensorflow_amd/dp.py: bind_to_gpu_numa). */
int fcn8s_device_pci_bus_id(int device_id, char* out, size_t len);
#define FCN8S_COMM_ID_BYTES 128
int fcn8s_comm_unique_id(void* id_out, size_t nbytes);
int fcn8s_comm_init(fcn8s_model* m, const void* unique_id, size_t nbytes, int rank, int world);
int fcn8s_comm_destroy(fcn8s_model* m);
int fcn8s_comm_info(const fcn8s_model* m, int* rank, int* world, int* rccl_version);   /* world = 0 without a communicator */
int fcn8s_allreduce_bucket(fcn8s_model* m, int bucket);
int fcn8s_comm_wait(fcn8s_model* m);
int fcn8s_comm_broadcast_params(fcn8s_model* m, int root);
int fcn8s_comm_allreduce_metrics(fcn8s_model* m);

/* ---- asynchronous host boundary (the reference's feed_dict copies, :558-560, are synchronous inside sess.run) ----------------
 * fcn8s_stage_inputs copies one host batch (images [N,H,W,3] uint8/float32, optional uint8 class ids [N,H,W]) into pinned
 * staging memory and starts the host-to-device copy on the model's own copy stream; it returns as soon as the copy is queued and
 * may be called from a feeder thread while the model's stream is busy with the previous step.  The device pointers it returns
 * are then fed to fcn8s_train_step / fcn8s_eval_step / fcn8s_predict with where = FCN8S_DEVICE, bracketed by fcn8s_stage_wait
 * (the model's stream waits for the copy) and fcn8s_stage_release (marks the point after which the slot may be refilled).
 * FCN8S_NUM_STAGE_SLOTS slots; refilling a slot waits for its previous release.                                              */
int fcn8s_stage_inputs(fcn8s_model* m, int slot, const void* images, int image_dtype, const uint8_t* label_ids,
                       int N, int H, int W, void** images_dev, uint8_t** labels_dev);
int fcn8s_stage_wait(fcn8s_model* m, int slot);
int fcn8s_stage_release(fcn8s_model* m, int slot);

/* ---- evaluation: sess.run(metric_update_ops) :685-689; reset :674; values :692 */
int fcn8s_eval_step(fcn8s_model* m, const void* images, int image_dtype, const uint8_t* label_ids,
                    int N, int H, int W, float l2_rate, int where);
int fcn8s_metrics_reset(fcn8s_model* m);
int fcn8s_metrics_get(fcn8s_model* m, double* mean_loss, double* mean_iou, double* accuracy);
/* all_classes != 0: mean IoU over ALL classes, an absent class counting as IoU 0 -- what tf.metrics.mean_iou of the tutorial's
 * TensorFlow 1.3.0 computes (fcn8s_tensorflow.py:291-293, fcn8s_tutorial.ipynb:311); 0: mean over the classes that occur in the
 * labels or the predictions (later TF 1.x; = fcn8s_metrics_get).  Identical whenever every class occurs.                        */
int fcn8s_metrics_get_ex(fcn8s_model* m, double* mean_loss, double* mean_iou, double* accuracy, int all_classes);
/* raw accumulators (for cross-rank reduction): confusion[C*C] row = label, col = prediction */
int fcn8s_metrics_raw(fcn8s_model* m, int64_t* confusion, double* loss_sum, int64_t* loss_count);
int fcn8s_metrics_set_raw(fcn8s_model* m, const int64_t* confusion, double loss_sum, int64_t loss_count);

/* ---- prediction: sess.run(predictions_argmax | softmax_output) :764-770 ---- *
 * argmax != 0: out = int64 [N,H,W]; else out = float32 softmax [N,H,W,C].        */
int fcn8s_predict(fcn8s_model* m, const void* images, int image_dtype, int N, int H, int W,
                  int argmax, void* out, int where);
/* ---- multi-scale / left-right-flip prediction (test-time augmentation) on images of any size ---------------------------------------- *
 * images: N same-size images [N,H,W,3], H, W >= 1; scales: nscales (1..8) factors in (0, 4]; P = nscales * (1 + flip) passes: for each
 * scale in order one pass, then (flip) its mirror image.  Pass of scale s: Hs = max(1, floor(H s + 0.5)), Ws likewise; the image is resized
 * to Hs x Ws (cv2.resize INTER_LINEAR on uint8, bit-exact with fcn8s_op_resample_u8), mirrored (flipped pass), preprocessed and padded bottom /
 * right to Hp x Wp = 32 ceil(Hs / 32) x 32 ceil(Ws / 32) with zeros in the preprocessed domain (the VGG mean colour); the predict forward of
 * the current precision mode runs on it; its logits over [0,Hs)x[0,Ws), un-mirrored, are resized to H x W bilinearly with half-pixel
 * centres (F.interpolate(mode='bilinear', align_corners=False)) and softmaxed.  out = the mean of the P softmaxes (summed in pass order in
 * fp32): float32 [N,H,W,C], or (argmax != 0) its int64 argmax [N,H,W] (lowest index on ties).  scales = {1}, no flip, H and W multiples of
 * 32: exactly fcn8s_predict.  float32 images are taken only when no pass resizes.  All passes share one workspace sized for the largest;
 * a repeated identical call allocates and frees nothing (statistic "workspace_allocations").  The parameters are treated as frozen for the
 * call (each transformed filter bank is built once); the model's frozen state is unchanged afterwards.  A model that is not frozen keeps
 * the banks' storage between calls with their contents marked stale: every call rebuilds them once, into that storage.
 * FCN8S_ERR_BAD_ARG: nscales outside 1..8, a scale outside (0, 4] or not finite, float32 images with a resizing pass;
 * FCN8S_ERR_SHAPE: a pass's padded shape cannot be planned. */
int fcn8s_predict_tta(fcn8s_model* m, const void* images, int image_dtype, int N, int H, int W, const float* scales, int nscales, int flip,
                      int argmax, void* out, int where);

/* ---- mean-field CRF refinement of a prediction (inference only; off unless asked for) ------------------------------------------------ *
 * A locally connected conditional random field over the softmax whose pairwise term looks at the colours of the input image (the local
 * window of Teichmann & Cipolla, "Convolutional CRFs", 2018; Potts compatibility).  Per image: probabilities P [H,W,C] (float32) and the
 * uint8 RGB image I [H,W,3] of the same size.  For pixel i and every offset (dy, dx) in {-r..r}^2 * d other than (0, 0) whose neighbour
 * j = i + (dy, dx) lies inside the image (neighbours outside contribute nothing, anywhere):
 *     s2   = dy^2 + dx^2                      c2 = sum_rgb (I_i - I_j)^2                  (exact integers)
 *     a_ij = exp(-s2 / (2 theta_alpha^2))                                                   (position only)
 *     k_ij = exp(-s2 / (2 theta_alpha^2) - c2 / (2 theta_beta^2))                           (appearance)
 *     g_ij = exp(-s2 / (2 theta_gamma^2))                                                   (smoothness)
 *     U_i(l) = log(max(P_i(l), FLT_MIN)),   Q^0 = P
 *     m_i(l) = w_appearance * sum_j k_ij Q_j^{t-1}(l) / sum_j a_ij  +  w_smooth * sum_j g_ij Q_j^{t-1}(l) / sum_j g_ij
 *     Q_i^t  = softmax_l(U_i(l) + m_i(l)),   t = 1 .. iterations, all pixels at once (Jacobi)
 * Both messages are divided by POSITION-ONLY sums: each lies in [0, 1] * w, a pixel with no similar neighbour receives almost no
 * appearance message, and a pixel at the border is treated like one in the interior.  A pixel with no neighbour inside the image has m = 0.
 * iterations = 0 returns P untouched, bit for bit.  The thetas and weights are float32; 1 / (2 theta^2) is formed in fp32.
 * Accepted: iterations 0..32 (default 5), radius 1..7 (3), dilation 1..8 (1), w_appearance (4) and w_smooth (2) finite and >= 0,
 * theta_alpha (8, pixels), theta_beta (13, colour units of 0..255) and theta_gamma (3, pixels) finite and > 0.  The defaults are a
 * starting point in the usual range of the dense-CRF literature; their effect on a trained model's mean IoU has not been measured. */
typedef struct fcn8s_crf_params {
    int32_t iterations, radius, dilation;
    float w_appearance, w_smooth, theta_alpha, theta_beta, theta_gamma;
} fcn8s_crf_params;
/* fcn8s_predict_tta with these arguments, followed by the mean field on its mean softmax (formed internally also when argmax != 0) and the
 * caller's uint8 images at H x W: out = Q^T float32 [N,H,W,C], or (argmax != 0) its int64 argmax [N,H,W] (lowest index on ties).
 * crf_params == NULL or iterations == 0: the result of fcn8s_predict_tta, bit for bit.  The CRF's buffers belong to the model's workspace:
 * a repeated identical call allocates and frees nothing ("workspace_allocations").  Profile group "crf_meanfield" (one entry per update).
 * FCN8S_ERR_BAD_ARG (the text names the field): a field outside the ranges above (NaN included), float32 images with iterations > 0
 * (the colours must be the uint8 ones), whatever fcn8s_predict_tta refuses; nothing is launched then. */
int fcn8s_predict_crf(fcn8s_model* m, const void* images, int image_dtype, int N, int H, int W, const float* scales, int nscales, int flip,
                      const fcn8s_crf_params* crf_params, int argmax, void* out, int where);

/* ---- Monte-Carlo dropout inference: the mean prediction and per-pixel uncertainty maps ------------------------------------------------ *
 * (Gal & Ghahramani 2016; Kendall et al., "Bayesian SegNet", 2015; Kendall & Gal 2017.)  Dropout stays on behind fc6 and fc7 at test time,
 * S stochastic passes are drawn and their softmaxes averaged.
 * images: N same-size images [N,H,W,3], H, W >= 1, uint8 or float32; samples = S in 1..FCN8S_MC_MAX_SAMPLES; keep_prob in (0, 1];
 * sample_offset = o >= 0 with o + S <= 2^30.  The image is preprocessed and padded bottom / right to multiples of 32 with zeros in the
 * preprocessed domain, exactly as the scale-1, unmirrored pass of fcn8s_predict_tta (H and W multiples of 32: fcn8s_predict's input path);
 * nothing is resized.  Sample s = 0 .. S-1: the prediction forward of the current precision mode with dropout behind fc6 and fc7 in the
 * training step's arithmetic (ReLU output times mask / keep_prob); fc6's mask is launch_dropout_mask(keep_prob, seed, stream) with the model's seed
 * on counter stream 0x80000000 + 2 (o + s), fc7's on that stream + 1 -- disjoint from training's streams 2 step and 2 step + 1 (step < 2^30), so
 * no call replays a training mask.  keep_prob = 1 draws no mask: every sample is the plain prediction.  Only fc6 and fc7 are stochastic: conv1_1 ..
 * pool5 and the pool3 / pool4 score heads run ONCE per call, fc6 -> fc7 -> decoder once per sample.
 * Per pixel, C classes, logits l_s of sample s, fp32 throughout, natural logarithm:
 *     p_s  = softmax(l_s) = expf(l_s - max) / sum                       h(p) = -sum_c p_c logf(max(p_c, FLT_MIN))      (folded in class order)
 *     mean = (sum_s p_s) * (1 / S)           summed in sample order, then one multiply by the fp32 reciprocal
 *     entropy            = h(mean)                                      the total predictive uncertainty
 *     mutual_information = max(0, entropy - (sum_s h(p_s)) * (1 / S))    its epistemic part (BALD): what the samples disagree about
 *     argmax of mean, lowest index on ties
 * out = the mean, float32 [N,H,W,C], or (argmax != 0) its int64 argmax [N,H,W], or NULL; entropy_out, mi_out = float32 [N,H,W] or NULL.
 * The two accumulators and the host staging belong to the model and only grow: a repeated identical call allocates nothing
 * ("workspace_allocations").  The parameters are treated as frozen for the call, as in fcn8s_predict_tta, and the model's frozen state is
 * unchanged afterwards.  After the call fcn8s_get_dropout_masks reports the masks of the call's LAST sample.  Profile group "mc_accumulate",
 * one entry per sample.  Two identical calls give identical bits.
 * FCN8S_ERR_BAD_ARG: samples, keep_prob or sample_offset out of range; out, entropy_out and mi_out all NULL.  FCN8S_ERR_STATE: the fp8_infer
 * precision, whose fc6 / fc7 kernels have no dropout epilogue.  Nothing is launched then. */
#define FCN8S_MC_MAX_SAMPLES 256
int fcn8s_predict_mc(fcn8s_model* m, const void* images, int image_dtype, int N, int H, int W,
                     int samples, float keep_prob, int64_t sample_offset,
                     int argmax, void* out /* int64 [N,H,W] or float32 [N,H,W,C] */,
                     float* entropy_out /* [N,H,W] or NULL */, float* mi_out /* [N,H,W] or NULL */, int where);

/* ---- state that must round-trip: global_step :246,:526; Adam slots ---------- */
int64_t fcn8s_global_step(const fcn8s_model* m);
int     fcn8s_set_global_step(fcn8s_model* m, int64_t step);
int     fcn8s_get_opt_state(fcn8s_model* m, float* host_m, float* host_v, size_t nfloats);
int     fcn8s_set_opt_state(fcn8s_model* m, const float* host_m, const float* host_v, size_t nfloats);

/* ---- introspection for parity tests ----------------------------------------- *
 * names: "pool3","pool4","fc7","logits", "conv1_1"... (post-ReLU activations)     */
/* frozen = 1: the caller promises that the parameters stay constant (an evaluate() / predict loop, the reference's sessions never
 * train inside one, fcn8s_tensorflow.py:660-697, :743-770); the library then keeps the tensors it derives from them across calls
 * instead of rebuilding them per forward pass: the Winograd-transformed filter banks (per layer and tile), the bf16 relayouts of the
 * kernels (the bf16 modes, FCN8S_PREC_BF16_TRAIN included), the e4m3 weight banks (FCN8S_PREC_FP8_INFER), and the padded conv1_1 /
 * phase-packed transposed-convolution kernels.  Any library call that changes parameters or starts a training pass unfreezes; whoever
 * writes into an external parameter buffer (fcn8s_config.ext_params) must call this with 0 first.  A writer who does not is caught by
 * a fingerprint of the parameter buffer, taken at the head of every frozen pass that reuses a kept tensor of ANY of these kinds and
 * compared at its end (off the critical path): on a mismatch all of them are dropped and the pass is run again without them. */
int fcn8s_freeze_params(fcn8s_model* m, int frozen);

/* Arithmetic mode (FCN8S_PREC_*); not in the reference, which is fp32 throughout.
 * BF16_FC needs fc6/fc7 widths that are multiples of 128 and a conv5 width that is a multiple of 32 (BAD_ARG otherwise). */
int fcn8s_set_precision(fcn8s_model* m, int precision);
int fcn8s_get_precision(const fcn8s_model* m);

/* FCN8S_PREC_FP8_INFER calibration.  fcn8s_fp8_calibrate (in that mode) runs the model's fp32 forward pass on the batch (keep_prob 1, direct
 * convolutions: every FP8 layer's input is materialised) and records per FP8 layer the maximum of |input| (an order-independent max reduction:
 * deterministic); calls accumulate the maximum until one with reset != 0 starts over.  get / set: n == FCN8S_FP8_LAYERS floats (finite, >= 0);
 * get is FCN8S_ERR_STATE without a calibration. */
int fcn8s_fp8_calibrate(fcn8s_model* m, const void* images, int image_dtype, int N, int H, int W, int where, int reset);
int fcn8s_fp8_get_calibration(const fcn8s_model* m, float* amax, int n);
int fcn8s_fp8_set_calibration(fcn8s_model* m, const float* amax, int n);

/* Algorithm options (not in the reference).  They select between maintained variants of the same arithmetic so that a parity report can
 * separate Winograd round-off from summation order; the defaults are the measured winners and production code never sets them.
 *   model options (m != NULL; setting one drops the workspace and all cached filter banks):
 *     "winograd_min_cin"  64   3x3 layers with at least this many input channels run through Winograd; 0 = direct convolution everywhere
 *     "winograd_tile"     6    largest 3x3 output tile (6, 4 or 2); per layer the allowed tile with the fewest multiplies is used
 *     "winograd_tile_hires", "winograd_hires_pixels"  0, 0   3x3 layers whose map has at least `hires_pixels` pixels per image use at most
 *                              tile `tile_hires` (F(4x4) carries half the round-off of F(6x6); the layers next to the input see the longest sums)
 *     "winograd_fc6"      1    fc6 as a 2x2 grid of 4x4 sub-filters through F(4x4,4x4); 0 = direct 7x7
 *     "fc6_fft"           1    (with winograd_fc6) fc6's forward + data gradient in the fp32 training step of an unfrozen model through 14x14
 *                              real-DFT tiles, 292 GEMM planes (fft_fc6.hip); 0 = F(4x4,4x4) there too
 *     "fc6_fft_wgrad"     1    (with fc6_fft) fc6's weight gradient in the same DFT domain when the step has at least 32 tiles of 8x8 (batch 4 at
 *                              1024x512); 2 = at any tile count; 0 = F(4x4,4x4)
 *     "tconv_gemm"        1    the 16x16/8 transposed conv as one GEMM over output blocks (blocked logits); 0 = 64 sub-pixel phases
 *     "fuse_dgrad_dout"   1    inside a VGG block the gather kernel of a conv's data gradient writes dM = A dZ A^T of the previous conv directly
 *                              (that conv's weight gradient and adjoint data gradient consume only dM): its dZ is never written; 0 = two kernels
 *     "fuse_out_in"       1    forward, inside a VGG block: the output transform of a conv is fused with the input transform of the next one (both
 *                              F(6x6,3x3) on the same tile grid): Y = relu(A^T M A + b) stays in registers / LDS and the kernel writes the next conv's
 *                              V = B^T d B (bit-identical to the two-kernel form); the conv's own activation tensor is then never written and
 *                              fcn8s_get_activation of it returns FCN8S_ERR_STATE (fcn8s_get_relu_record still answers).  0 = two kernels; 1 = fused unless the
 *                              launch would need row ranges of fewer than four tile rows per block to fill the chip (a single image, conv5_x: the
 *                              recomputed halo rows then eat the gain); 2 = fused whenever the shapes allow
 *     "bf16_gemm256"      1    FCN8S_PREC_BF16_FC: fc6 / fc7 forward on the 256 x 256 LDS-DMA kernel -- 0 never, 1 when the launch has at least
 *                              128 tiles (training batches), 2 whenever the shapes allow (rows and Cout multiples of 256)
 *     "conv1_tiled"       1    conv1_1 forward on the spatial-tile kernel (halo tile in LDS); 0 = the LDS-DMA gather kernel (bit-identical results)
 *     "conv1_wgrad_mfma"  1    conv1_1 weight gradient as a (27 -> 32) x 64 MFMA product over pixels; 0 = the VALU kernel
 *     "conv1_in_transform" 1   conv1_1 (3x3, 3 -> 64, bias, ReLU) is evaluated inside conv1_2's F(6x6,3x3) input transform, on that transform's own 8 x 8
 *                              patches and straight from the preprocessed image: conv1_1's activation tensor (134 MB per 1024x512 image) is never written
 *                              or read, fcn8s_get_activation("conv1_1") returns FCN8S_ERR_STATE (fcn8s_get_relu_record still answers in training).  Same
 *                              products in another summation order (VALU fma chain instead of the MFMA kernel's).  0 = conv1_1 as a kernel of its own
 *     "gemm_out_fused64"  1    forward: conv1_2 (64 -> 64, F(6x6,3x3), its output read by its pool alone) runs its 64 position GEMMs, the output
 *                              transform, bias, ReLU and the 2x2/2 max-pool with its argmax bytes in one kernel (wino_gemm_out64_kernel): the layer's
 *                              Winograd-domain output (3.86 GB at 16 x 1024x512) is never written.  The same fma chains as the output transform behind
 *                              a GEMM of another summation order: results agree with the two-kernel route to round-off.  Only FCN8S_PREC_F32
 *                              takes it: a launch under any other precision runs the two kernels.  Like the other route options it drops the workspace and the kept filter banks when it
 *                              changes.  0 = position GEMM + output transform
 *     "bf16_copy_by_transform" 1  FCN8S_PREC_BF16_FWD / _X2, training: the padded bf16 copy of a layer's input that its direct bf16 convolution reads is
 *                              written by the layer's Winograd input transform (which runs anyway, for the weight gradient) instead of a
 *                              conversion pass of its own over the activations (identical bits); 0 = the separate pass
 *     "deterministic"     0    1 = every reduction that the default path splits over blocks and joins with fp32 atomics (weight gradients in and out of
 *                              the Winograd domain, conv1_1's and the score heads' weight gradients, the bf16 weight gradients, the last bias gradient, the L2
 *                              sum; split-K GEMMs are simply not split) stores one partial result per split into a scratch slab, and a second kernel adds
 *                              the slabs in split order: two runs of the same steps on the same inputs give the same bits.  +2.4 % at 16 x 1024x512
 *     "bf16_acts"         1    FCN8S_PREC_BF16_TRAIN, training passes: a tensor between two bf16 convolutions exists only as the consumer's padded bf16 copy -- written by the
 *                              producer's epilogue (conv -> conv activations, conv1_1 included; the last convolutions of blocks 1, 2, 5, which their pools read as
 *                              bf16 copies -- maxima and gradient routing among the bf16 values; the pooled maps pool1 / pool2 / pool5; the output gradient of a conv that
 *                              follows a bf16 conv, together with that layer's bias gradient).  fcn8s_get_activation of such a layer then returns FCN8S_ERR_STATE naming
 *                              this option; 0 keeps every fp32 tensor too (same values into every product: bit-identical losses and weight gradients)
 *     "bf16_fuse_pool"    1    FCN8S_PREC_BF16_TRAIN: the forward pools keep routing bytes (and write their consumer's bf16 copy), the max-pool backward kernel reads those bytes and
 *                              writes the last conv's padded bf16 dZ copy and bias gradient itself; 0 = plain pools + conversion passes
 *     "bf16_rows_bn"      0    FCN8S_PREC_BF16_TRAIN: 128 = the flat-position 3 x 3 convolution kernel takes its 128-column tile where it can (A/B; slower)
 *     "bf16_infer_copies" 1    FCN8S_PREC_BF16_TRAIN: evaluation / prediction passes take the training pass's data flow (padded bf16 copies written by the producers' epilogues, the
 *                              flat-position kernel, pools on the bf16 copies; logits = the training pass's, bit for bit); 0 = fp32 tensors converted layer by layer (round 5)
 *     "keep_output_gradients" 0 (tests) every weighted layer's fp32 output gradient dY is copied as the backward pass hands it to the layer's weight gradient and can be read with
 *                              fcn8s_get_activation(m, "dy:<layer>", ...) (conv1_1 .. conv5_3, fc6, fc7); FCN8S_ERR_STATE for a layer whose gradient travelled in another form
 *                              (these ten pick a kernel per launch and drop nothing)
 *     "workspace_allocations"  (read-only statistic; setting it is FCN8S_ERR_BAD_ARG) device allocations the model has made for its workspace,
 *                              the scratch of fcn8s_predict_tta and fcn8s_predict_crf, its bf16 copies and its cached (frozen / TTA) filter banks
 *     "frozen"                 (read-only) 1 while fcn8s_freeze_params(m, 1) holds
 *     "device_bytes_live"      (read-only, process-wide: m may be NULL) device bytes the library's models and op-level calls hold right now (not the per-stream scratch)
 *     "scratch_bytes_live"     (read-only, process-wide: m may be NULL) device bytes of the per-(device, stream) scratch (slab reductions, column sums, split-K
 *                              slabs) held right now.  A model's fcn8s_destroy releases the scratch of every stream it ran on; op-level calls have no owner, so
 *                              what they grow on a stream stays until a model that ran on that stream is destroyed: at most two buffers per distinct stream
 *     "comm_timeout_ms" 600000 the communicator's watchdog (see fcn8s_comm_init): a collective older than this is given up, the communicator aborted
 *   op-context options (m == NULL): the arithmetic of the op-level entry points below, which have no model.  The value belongs to the
 *   CALLING THREAD (thread-local) and is read by that thread's later fcn8s_op_* calls only; no model ever reads it, so two models -- or a
 *   feeder thread beside a compute thread -- cannot change each other's kernels:
 *     "op_f32x3"          0    their LDS-DMA GEMMs use the split-bf16 arithmetic of FCN8S_PREC_F32X3
 *     "op_split_pieces"   0    the same switch by piece count: 0 = f32 MFMA, 3 = FCN8S_PREC_F32X3, 2 = FCN8S_PREC_F32X2
 *     "op_bf16_planes"    1    fcn8s_op_conv2d_bf16_train keeps its padded bf16 copies as channel-chunk planes [C / 32][rows][32] (what FCN8S_PREC_BF16_TRAIN does);
 *                              0 = [rows][C], the layout the kernels also take (same results)
 *     "op_bf16_rows_bn"   0    the same switch ("bf16_rows_bn": 0 / 64 = 256 x 64 blocks, 128 = 128 x 128) for fcn8s_op_conv2d_bf16_train
 *     "op_gemm_out_fused64" 0  fcn8s_op_conv3x3_winograd_fwd_bwd and fcn8s_op_conv3x3_winograd_pool ask for the route of "gemm_out_fused64" (their bare models set the
 *                              layer's fact and the option; whether wino_gemm_out64_kernel then runs stays the launch's own decision: 64 -> 64 channels, tile 6,
 *                              the fp32 arithmetic, the pool as the only output): 1 = asked for, 2 = the same with the kernel's non-temporal-store instantiation
 *                              whatever the size (a model launches it from 64e6 pooled bytes up), 0 = position GEMM + output transform.  Other values: FCN8S_ERR_BAD_ARG
 *     "op_deterministic"  0    the slab reductions of "deterministic" for the op-level entry points (a model call on the same thread sets the
 *                              thread's switch from that model's option: set it again before the next op-level call)
 *     "op_poison_scratch" 0    for tests: while 1, every hand-out of the two per-(device, stream) scratch pools (split-K slabs, slab reductions, column-sum
 *                              partials) is filled with 0xFF bytes -- fp32 NaNs -- on the caller's stream first, so a consumer that reads what its producer
 *                              did not write gets a NaN instead of an earlier call's leftovers.  Results do not change; every hand-out costs a fill.  (The
 *                              pools are shared code: a model call made on the same thread while the option is 1 gets the fill too.)
 *     "op_scratch_poisoned_bytes"  (read-only) the bytes so filled on this thread since "op_poison_scratch" was last set
 * Unknown keys return FCN8S_ERR_NOT_FOUND. */
int fcn8s_set_option(fcn8s_model* m, const char* key, int64_t value);
int fcn8s_get_option(const fcn8s_model* m, const char* key, int64_t* value);

int fcn8s_get_activation(fcn8s_model* m, const char* name, float* host, size_t nfloats);
int fcn8s_get_dropout_masks(fcn8s_model* m, float* host_mask6, size_t n6, float* host_mask7, size_t n7);
/* Parity instrumentation (no counterpart in the reference): which element of each 2x2 window the backward pass of pool `block` (1..5)
 * routes the gradient to -- one byte per pooled element [N, h/2, w/2, c]: 0..3 = window element (2*row + col) holding the FIRST maximum,
 * 4 = the maximum is not > 0 (ReLU off: no gradient).  Max-pool's argmax is discontinuous at ties; the checker differentiates along
 * the recorded routes and verifies separately that every route that differs from its own is a tie to round-off.  Valid after a
 * training forward pass (fcn8s_forward_loss / fcn8s_train_step). */
int fcn8s_get_pool_routing(fcn8s_model* m, int block, unsigned char* host, size_t nbytes);
/* Parity instrumentation: the ReLU record the backward pass masks with, one byte (0 / 1) per element [N,h,w,c] of a conv that feeds another
 * conv ("conv1_1" .. "conv5_2") -- what `activation > 0` says when the activation exists; with "fuse_out_in" the activation of such a layer
 * is never written and this record is all there is.  Valid after a training forward pass whose layer kept a record (Winograd layers). */
int fcn8s_get_relu_record(fcn8s_model* m, const char* layer, unsigned char* host, size_t nbytes);

/* ---- host helper for the TF tensor-bundle writer (tf_bundle.py): CRC-32C (Castagnoli) of a host buffer ----- */
uint32_t fcn8s_crc32c(const void* data, size_t nbytes, uint32_t crc);

/* ---- in-library HIP-event timing of kernel groups (bench.py roofline) -------- *
 * groups: "conv3x3_fwd","conv3x3_dgrad","conv3x3_wgrad","fc_fwd","fc_dgrad","fc_wgrad",...
 * Fills total milliseconds, number of launches, algorithmic flops and bytes.
 * fcn8s_profile_enable(m, 2) splits the conv groups per layer ("conv3x3_fwd:conv1_2"), and adds count-only groups "derived:<build step>"
 * (launches only; ms, flops and bytes are 0 -- skip them before dividing by ms) for every tensor a forward pass (re)builds from the
 * parameters alone.  The suffix names the build step, written at its call site, not necessarily one kernel: "derived:wino_filter_kernel",
 * "derived:w_to_bf16_t_kernel", "derived:w_to_bf16_tiles_kernel", "derived:prepare_forward_weights" (the padded conv1_1 and phase-packed
 * transposed-convolution kernels, four launches) -- what the later passes of a frozen model report as zero.  */
int fcn8s_profile_enable(fcn8s_model* m, int on);
int fcn8s_profile_reset(fcn8s_model* m);
int fcn8s_profile_num_groups(const fcn8s_model* m);
int fcn8s_profile_get(fcn8s_model* m, int group, const char** name, double* total_ms,
                      int64_t* launches, double* flops, double* bytes);

/* ---- single ops on DEVICE pointers (unit parity tests; same kernels the model
 * uses).  `stream` may be NULL (default stream).  Every entry needs no ordering but
 * that of `stream` (an entry that returns a value to the host synchronises `stream`,
 * then copies with a blocking hipMemcpy).  The scratch such a call grows
 * for `stream` has no owner (see "scratch_bytes_live"): bounded by the number of
 * distinct streams.                                                               */
int fcn8s_op_preprocess(void* stream, const void* images, int image_dtype, float* out4, int64_t npix);
/* the two kernels of fcn8s_predict_tta on DEVICE pointers.  tta_input: uint8 [N,H,W,3] -> the forward's input [N,Hp,Wp,4] (resize to
 * Hs x Ws as fcn8s_op_resample_u8, mirror if flip, fcn8s_op_preprocess's arithmetic, zeros outside [0,Hs)x[0,Ws)).  tta_accumulate: plain
 * NHWC logits [N,Hp,Wp,C] over [0,Hs)x[0,Ws), un-mirrored if flip, bilinear (half-pixel) to H x W, softmax; first: acc = p, else acc += p;
 * last: (acc + p) / npasses into softmax_out [N,H,W,C] and / or argmax_out [N,H,W] (acc is then not written; it may be NULL if first and
 * last).  16-byte aligned float pointers. */
int fcn8s_op_tta_input(void* stream, const uint8_t* images, int N, int H, int W, int Hs, int Ws, int Hp, int Wp, int flip, float* out4);
int fcn8s_op_tta_accumulate(void* stream, const float* logits, int N, int Hp, int Wp, int Hs, int Ws, int flip, int C, int H, int W, float* acc,
                            int first, int last, int npasses, float* softmax_out, int64_t* argmax_out);
/* fcn8s_predict_mc's kernel on DEVICE pointers: one sample's plain logits [N,H,W,C] into the running sums acc [N,H,W,C] and ent_acc [N,H,W]
 * (`first` stores instead of adding; `last` writes no accumulator but every output that is not NULL: the mean softmax, its int64 argmax, its
 * entropy, the mutual information -- the definition is at fcn8s_predict_mc).  first && last (S = 1) touches no accumulator: both may be NULL. */
int fcn8s_op_mc_accumulate(void* stream, const float* logits /*[N,H,W,C] plain*/, int N, int H, int W, int C,
                           float* acc, float* ent_acc, int first, int last, int nsamples,
                           float* softmax_out, int64_t* argmax_out, float* entropy_out, float* mi_out);   /* any output may be NULL */
/* the mean field of fcn8s_predict_crf on DEVICE pointers (definition: at fcn8s_crf_params): prob, q_out float32 [N,H,W,C] (16-byte aligned,
 * C a multiple of 4), images uint8 [N,H,W,3]; work: scratch of fcn8s_op_crf_work_floats(N, H, W, C, p) floats (may be NULL when that is
 * 0); q_out (Q^T) and argmax_out (int64 [N,H,W]) may each be NULL, not both.  prob is not written and may not overlap work or q_out.
 * FCN8S_ERR_BAD_ARG for a field of p outside its range (the text names it), FCN8S_ERR_SHAPE if C floats of a tile do not fit the LDS
 * (C <= 52 fits at every radius). */
size_t fcn8s_op_crf_work_floats(int N, int H, int W, int C, const fcn8s_crf_params* p);
int fcn8s_op_crf_meanfield(void* stream, const float* prob, const uint8_t* images, int N, int H, int W, int C, const fcn8s_crf_params* p,
                           float* work, float* q_out, int64_t* argmax_out);
/* GPU-side augmentation of a uint8 batch on DEVICE pointers (the crop / canvas placement, horizontal flip and
 * brightness steps of data_generator/batch_generator.py:293-341, :469-486, which do not resample).  params: int32[4] per image =
 * {y offset, x offset, flip (0|1), brightness (0|1)}; out[n,y,x] = in[n, y+oy, (flip ? Wo-1-x : x) + ox], zero / void_id outside the
 * source.  Brightness is the reference's `_brightness` in OpenCV's 8-bit arithmetic (cv2.COLOR_RGB2HSV integer path, V replaced through
 * vlut[n][V] -- uint8[N][256], the host's evaluation of `V * random_br` saturated at 255 and truncated --, cv2.COLOR_HSV2RGB float32 path);
 * bit-exact with fcn8s_tensorflow_amd/cv2_compat.py.  labels / out_labels / vlut may be NULL. */
int fcn8s_op_augment_u8(void* stream, const uint8_t* images, const uint8_t* labels, uint8_t* out_images, uint8_t* out_labels,
                        const int32_t* params, const uint8_t* vlut, int N, int H, int W, int Ho, int Wo, int void_id);
/* the resampling augmentations of data_generator/batch_generator.py:328-384 (resize :328-331, translate :344-356, scale :358-384) on
 * DEVICE uint8 batches: image n is resized to params[4n+0] x params[4n+1] -- images as cv2.resize(INTER_LINEAR) does for 8-bit data (11-bit
 * fixed-point taps; 2x2 box mean for an exact 2x shrink), labels as cv2.resize(INTER_NEAREST) does (floor(dst * src/dst)) -- and placed at
 * offset (params[4n+2], params[4n+3]) of the [Ho,Wo] output, uncovered pixels 0 / void_id.  Bit-exact with cv2_compat.py.
 * images / labels may each be NULL. */
int fcn8s_op_resample_u8(void* stream, const uint8_t* images, const uint8_t* labels, uint8_t* out_images, uint8_t* out_labels,
                         const int32_t* params, int N, int H, int W, int Ho, int Wo, int void_id);
int fcn8s_op_conv2d(void* stream, const float* x, const float* w_hwio, const float* bias, float* y,
                    int N, int H, int W, int Cin, int Cout, int K, int relu);
/* the same SAME conv through Winograd F(tile x tile, 3x3), tile = 2, 4 or 6 (the path the model takes for its 3x3
 * layers; tile 6 handles partial edge tiles, tiles 2 and 4 need H, W multiples of tile; K = 7 with tile 4 runs fc6's
 * decomposition into 4x4 sub-filters, F(4x4,4x4)) */
int fcn8s_op_conv2d_winograd(void* stream, const float* x, const float* w_hwio, const float* bias, float* y,
                             int N, int H, int W, int Cin, int Cout, int K, int relu, int tile);
/* One 3x3 SAME conv + bias + ReLU the way the model's 3x3 layers run in a TRAINING step, forward and backward, through the model's own
 * launch sequences (Winograd F(tile x tile, 3x3), tile = 2, 4 or 6; Cin, Cout multiples of 64):
 *   forward   y = relu(conv(x, w) + bias), keeping the transformed input V and the filter bank U; pooled != 0: the output transform
 *             also writes pool = maxpool2x2(y) [N,H/2,W/2,Cout] and one argmax byte per window (y may then be NULL: a block's last
 *             conv output is never materialised);
 *   backward  dy = gradient w.r.t. the PRE-activation [N,H,W,Cout] (pooled == 0), or w.r.t. the pool output [N,H/2,W/2,Cout]
 *             (pooled != 0: max-pool and ReLU backward happen inside the transform, routed by the argmax bytes);
 *             dM = A dY A^T once; dw = Winograd-domain weight gradient V^T dM; db from dM's (1,1) slab; dx = data gradient, for tile 6
 *             as the adjoint of the forward algorithm (dV = dM U^T on the transposed-B GEMM, overlap-add gather), for tiles 2 / 4 as a
 *             forward-type Winograd conv on flipped filters; + dx_addend (optional skip gradient), then masked by (x > 0) if
 *             mask_mode = 1 (x read as the mask) or 2 (one-bit record written by this conv's input transform, the conv1_1 case).
 * With op context "op_gemm_out_fused64" on, y == NULL, pooled != 0, tile 6 and 64 -> 64 channels the forward is wino_gemm_out64_kernel (conv1_2's route).
 * Not in the reference; exists so that the Winograd backward has op-level parity tests. */
int fcn8s_op_conv3x3_winograd_fwd_bwd(void* stream, const float* x, const float* w_hwio, const float* bias, const float* dy, const float* dx_addend,
                                      float* y, float* pool, float* dx, float* dw, float* db,
                                      int N, int H, int W, int Cin, int Cout, int tile, int pooled, int mask_mode);
/* One 3x3 SAME conv + bias + ReLU + 2x2/2 max-pool the way the LAST conv of a block runs forward, through the model's own launch sequence (Winograd
 * F(tile x tile, 3x3), tile = 4 or 6; Cin, Cout multiples of 64; even H, W, multiples of 4 for tile 4): pool = maxpool2x2(relu(conv(x, w) + bias))
 * [N,H/2,W/2,Cout]; the full-resolution output is never written.
 *   train != 0  a training pass: V is kept in the layer's own slot, the filter bank for the step, and pidx (device, one byte per pooled element, may be
 *               NULL) receives the argmax bytes of fcn8s_get_pool_routing;
 *   train == 0  an inference pass (fcn8s_predict): V goes to the shared scratch, the bank to the filter-bank scratch, pidx is not written.
 *   fused (host, may be NULL) receives 1 if wino_gemm_out64_kernel was launched (op context "op_gemm_out_fused64" asks for it; the launch decides), else 0.
 * Every scratch buffer (V, M, the filter bank with room for the second copy behind it, the kept V) is an allocation of its own, filled with NaNs before
 * the call.  Not in the reference; for tests only -- it allocates and synchronises per call, so it says nothing about time. */
int fcn8s_op_conv3x3_winograd_pool(void* stream, const float* x, const float* w_hwio, const float* bias, float* pool, unsigned char* pidx,
                                   int N, int H, int W, int Cin, int Cout, int tile, int train, int* fused);
/* One 7x7 SAME conv the way fc6 runs in an fp32 TRAINING step, forward and backward, through the model's own launch sequences and under the
 * model's own rules for which kernels take a shape (Cin % 16 == 0, Cout % 128 == 0):
 *   forward   y = dropout(relu(conv(x, w) + bias)); bias may be NULL; dropout only if keep_prob < 1, with `seed` and the Philox stream fc6 has in a
 *             model's first step (element index NHWC, survivors scaled by 1 / keep_prob);
 *   backward  dy = gradient w.r.t. the PRE-activation [N,H,W,Cout]; dw, db (may be NULL) and dx are assigned, not accumulated;
 *   path      0 = option fc6_fft off: F(4x4,4x4) sub-filter Winograd where H and W are multiples of 4, else the direct kernels;
 *             1 = forward and data gradient through the 14x14 real-DFT tiles, weight gradient outside the DFT domain (fc6_fft_wgrad = 0: what a
 *                 model does below 32 tiles);  2 = fc6_fft_wgrad = 2: the weight gradient in the DFT domain too.
 *             A path only permits: a map on which the DFT tiles multiply more than the alternative, a width the transposed-B GEMM does not take, or
 *             a split-bf16 op context (option op_split_pieces; the DFT path is fp32 only) run what a model would run there.
 *   dft_products (host, may be NULL) receives the products that did run in the DFT domain: bit 0 forward, bit 1 weight gradient, bit 2 data gradient.
 * The scratch (wino_v, wino_m, the layer's wv slot, the filter-bank scratch) has exactly the sizes a model plans for this shape and is filled with
 * NaNs before the forward pass, as a stand-in for the other layers' leftovers a model's shared workspace holds behind a slab or a partial row tile.
 * keep_prob in (0, 1].  Not in the reference; for tests only -- it allocates and synchronises per call, so it says nothing about time. */
int fcn8s_op_conv7x7_fc6_fwd_bwd(void* stream, const float* x, const float* w_hwio, const float* bias, const float* dy,
                                 float* y, float* dx, float* dw, float* db,
                                 int N, int H, int W, int Cin, int Cout, int path, float keep_prob, uint64_t seed, int* dft_products);
/* the same SAME conv with bf16-rounded operands and fp32 accumulation on the bf16 MFMA (FCN8S_PREC_BF16_FC's kernel);
 * Cin % 32 == 0, Cout % 128 == 0, K odd */
int fcn8s_op_conv2d_bf16(void* stream, const float* x, const float* w_hwio, const float* bias, float* y,
                         int N, int H, int W, int Cin, int Cout, int K, int relu);
/* One K x K SAME convolution in the arithmetic of FCN8S_PREC_BF16_TRAIN, on the kernels that mode runs: forward y = conv(bf16 x, bf16 w) + bias (ReLU if
 * relu), data gradient dx = conv^T(bf16 dy, bf16 w) (masked by `mask` > 0 if given), weight gradient dw = corr(bf16 x, bf16 dy), bias gradient
 * db = sum dy.  Any of y, dx, dw, db may be NULL (then x / dy / w are only needed for what is asked).  Cin, Cout % 64 == 0, K odd. */
int fcn8s_op_conv2d_bf16_train(void* stream, const float* x, const float* w_hwio, const float* bias, float* y, int relu,
                               const float* dy, const float* mask, float* dx, float* dw, float* db,
                               int N, int H, int W, int Cin, int Cout, int K);
/* One K x K SAME convolution in the arithmetic of FCN8S_PREC_FP8_INFER on that mode's kernel: x quantized with exponent x_exp (q(x 2^-x_exp)),
 * w per output channel (ew = E(max |w[..., co]|)), y = 2^(x_exp + ew) sum Xq Wq + bias (ReLU if relu; bias may be NULL).  Cin, Cout % 64 == 0, K odd. */
int fcn8s_op_conv2d_fp8(void* stream, const float* x, const float* w_hwio, const float* bias, float* y, int relu, int x_exp,
                        int N, int H, int W, int Cin, int Cout, int K);
int fcn8s_op_conv2d_bwd(void* stream, const float* x, const float* w_hwio, const float* dy,
                        float* dx, float* dw, float* db,
                        int N, int H, int W, int Cin, int Cout, int K);
int fcn8s_op_maxpool2x2(void* stream, const float* x, float* y, int N, int H, int W, int C);
int fcn8s_op_maxpool2x2_bwd(void* stream, const float* x, const float* dy, float* dx,
                            int N, int H, int W, int C, int relu_mask);
int fcn8s_op_conv2d_transpose(void* stream, const float* x, const float* w_kkoi, const float* bias,
                              const float* addend, float* y,
                              int N, int Hi, int Wi, int C, int K, int S);
int fcn8s_op_conv2d_transpose_bwd(void* stream, const float* x, const float* w_kkoi, const float* dy,
                                  float* dx, float* dw, float* db,
                                  int N, int Hi, int Wi, int C, int K, int S);
int fcn8s_op_softmax_xent(void* stream, const float* logits, const uint8_t* label_ids, float* dlogits,
                          float* loss_out_dev, int64_t npix, int C);
/* the weighted / OHEM loss of fcn8s_set_loss on plain [npix, C] logits (C <= 64), gradient scale 1/npix (weighted) or 1/|K| (OHEM).
 * class_weights_dev: device float[C] or NULL (all 1; not checked).  With NULL weights and ohem_thresh 0 this is fcn8s_op_softmax_xent.
 * pixel_loss_dev (OHEM only, may be NULL): float[npix], l_p of every valid pixel and -1 for an ignored one.  stats_dev (may be NULL;
 * untouched in the default case): int64[3] = |V|, |K| (|V| when weighted), the float bit pattern of t (0 when weighted).  Synchronises. */
int fcn8s_op_softmax_xent_ex(void* stream, const float* logits, const uint8_t* label_ids, const float* class_weights_dev,
                             float ohem_thresh, int64_t ohem_min_kept, float* dlogits, float* loss_out_dev,
                             float* pixel_loss_dev, int64_t* stats_dev, int64_t npix, int C);
/* Boundary-weighted cross-entropy, the kernels (a per-pixel weight by the distance to the nearest ground-truth boundary: U-Net's weight map
 * 1 + w0 exp(-d^2 / 2 sigma^2), Ronneberger et al., MICCAI 2015, or weight 0 in a band around the contours against the label noise of polygon
 * annotations).  fcn8s_set_boundary_loss switches the weighting on for a model's training losses (the model rule is stated there); these two
 * ops are its kernels on plain data.  Definitions, per image of a batch [N, H, W] of uint8 label ids.  Raw ids are compared: an id >= C ("ignore") is a label like
 * any other and a border towards it is a boundary (the rule of fcn8s_op_boundary_pair's trimap rings).  Pixels outside the image do not exist;
 * images do not see each other.
 *   d2(p) = min over q != p in the same image with y[q] != y[p] of |q - p|^2 (squared Euclidean pixel distance, an integer).
 *   Radius R, 1 <= R <= 15.  code(p) = d2(p) if d2(p) <= R^2 (1 .. 225), else 255: one byte (which is why R ends at 15, not at 16).
 *   b_p = table[code(p)], table = 256 floats of the caller's, each finite and >= 0; entries whose code cannot occur at this R are never read.
 *   Wherever fcn8s_set_loss's definition has w_{y_p}, the weight is w_p = fl32(w_{y_p} * b_p) -- one fp32 product; class weights default to 1:
 *   weighted (ohem_thresh == 0): L = (1/P) sum_{p in V} w_p l_p, dlogits_p = (w_p / P)(softmax_p - onehot_p), the denominator stays P;
 *   OHEM: the selection is made on the unweighted l_p as before; w_p scales the kept pixels in loss and gradient, denominator |K|.
 *   A table of all 1.0 gives the bits of the same configuration without a table.
 * fcn8s_op_softmax_xent_px = fcn8s_op_softmax_xent_ex with these weights: codes_dev = device uint8[npix] (a code per pixel, as
 * fcn8s_op_boundary_distance writes them; any byte is a valid index), table256_dev = device float[256] (not checked).  Both NULL:
 * fcn8s_op_softmax_xent_ex; exactly one NULL: FCN8S_ERR_BAD_ARG.  Synchronises. */
int fcn8s_op_softmax_xent_px(void* stream, const float* logits, const uint8_t* label_ids, const float* class_weights_dev,
                             float ohem_thresh, int64_t ohem_min_kept, const uint8_t* codes_dev, const float* table256_dev, float* dlogits,
                             float* loss_out_dev, float* pixel_loss_dev, int64_t* stats_dev, int64_t npix, int C);
/* the Lovász-softmax loss of fcn8s_set_lovasz on plain [nseg * seg_pixels, C] data (C <= 64): x = logits (x_is_logits = 1) or
 * probabilities (0; the errors are then taken from x itself); nseg segments of seg_pixels consecutive pixels each; class_mask_dev =
 * device uint8[C] or NULL (every class).  loss_out_dev[0] = L_lov; grad_out (may be NULL) = d L_lov / d x, zero rows for ignored pixels;
 * class_loss_out (may be NULL) = device float[nseg C], l_{s,c} (0 for a class outside C_s).  Synchronises. */
int fcn8s_op_lovasz_softmax(void* stream, const float* x, int x_is_logits, const uint8_t* label_ids, int64_t nseg, int64_t seg_pixels, int C,
                            int classes_all, const uint8_t* class_mask_dev, float* loss_out_dev, float* grad_out, float* class_loss_out);
int fcn8s_op_softmax_argmax(void* stream, const float* logits, float* softmax_out, int64_t* argmax_out,
                            int64_t npix, int C);
int fcn8s_op_confusion(void* stream, const uint8_t* label_ids, const int64_t* pred_ids, int64_t npix,
                       int64_t* conf, int C);
/* The counting half of the official Cityscapes pixel-level evaluation (cityscapesscripts/evaluation/evalPixelLevelSemanticLabeling.py with
 * evalInstLevelScore on, its default) for a batch of N images of P pixels each on DEVICE pointers, in one pass that reads every input byte once.
 *   gt_label_ids [N,P] uint8 label ids 0..33; gt_instance_ids [N,P] uint16 (*_gtFine_instanceIds.png: a plain label id below 1000, or
 *   label * 1000 + k), or NULL: confusion matrix only; pred [N,P]: pred_kind 0 = int64 train ids 0..19 as fcn8s_predict writes them, mapped to
 *   label ids inside the kernel (labels.py trainId -> id; 0 -> 0), pred_kind 1 = uint8 label ids 0..33.
 *   conf [34*34] int64: conf[gt * 34 + pred] += 1 for every pixel (the caller clears it; it accumulates over calls).
 *   Instance statistics (:595-635).  Counted labels: person 24, rider 25, car 26, truck 27, bus 28, train 31, motorcycle 32, bicycle 33; category
 *   id lists: human = {24, 25}, vehicle = {26 .. 33} (caravan 29 and trailer 30 belong to the list although their instances are skipped).  For every
 *   value v > 1000 (strictly) of an image's instance map with L = v / 1000 a counted label:
 *       size = #{inst == v},  tp = #{inst == v and pred == L},  cattp = #{inst == v and pred in ids(category(L))}
 *   (the mask is the instance map's alone; gt is not consulted).  v with an ignoreInEval label (1000 < v < 7000, 9xxx, 10xxx, 14xxx .. 16xxx, 18xxx,
 *   29xxx, 30xxx) is skipped as the evaluator skips it; v with an evaluated label that has no instances (7005, say) or with L > 33 is the
 *   evaluator's KeyError: such pixels are counted in counts[n][2] and the caller refuses the image.
 *   entries [N][max_entries][4] int32 = {v, size, tp, cattp} of image n in ascending v (np.unique's order); counts [N][3] int64 (written, not
 *   accumulated) = {number of entries found -- it may exceed max_entries, then only the first max_entries were written and the call is to be
 *   repeated with more room --, pixels whose gt or pred id is out of range (they are counted nowhere else), pixels of a bad v}.
 *   The host turns entries into the weighted sums in float64, in the evaluator's order (cityscapes_eval.py): weight = avgClassSize[L] / size,
 *   tpWeighted += tp * weight, fnWeighted += (size - tp) * weight, the category likewise with cattp; iIoU = tpW / (tpW + fp + fnW), fp from conf.
 * work: fcn8s_op_cityscapes_work_bytes(N) bytes of 16-byte aligned device scratch (may be NULL without an instance map).  Integers only: two
 * runs give the same bits.  Stream-ordered; does not synchronise.  FCN8S_ERR_BAD_ARG (nothing launched) for a NULL gt / pred / conf / counts,
 * pred_kind outside {0, 1}, N <= 0, P <= 0, max_entries < 0, or an instance map with NULL entries / work; FCN8S_ERR_SHAPE for P >= 2^31. */
size_t fcn8s_op_cityscapes_work_bytes(int N);
int fcn8s_op_cityscapes_pair(void* stream, const uint8_t* gt_label_ids, const uint16_t* gt_instance_ids, const void* pred, int pred_kind,
                             int N, int64_t P, int64_t* conf, void* work, int32_t* entries, int max_entries, int64_t* counts);
/* The counting half of the calibration and error-detection measures of a softmax against its ground truth (expected calibration error and
 * reliability diagram: Guo et al., ICML 2017; NLL and Brier score; AUROC / AUPR / risk-coverage of "uncertainty predicts a wrong pixel":
 * Hendrycks & Gimpel, ICLR 2017, Geifman & El-Yaniv, NeurIPS 2017) for a batch of N images of P pixels each on DEVICE pointers, in one pass that
 * reads every input byte once.  The measures themselves are taken from the tables in float64 on the host (reliability.py).
 *   prob [N,P,C] float32, as fcn8s_predict (argmax = 0), fcn8s_predict_tta, fcn8s_predict_crf and fcn8s_predict_mc write it; any C >= 2 and any
 *   float alignment (16-byte loads are used when the pointer is 16-byte aligned and C % 4 == 0).  gt [N,P] uint8, any alignment; lut: 256 uint8 on
 *   the device.  scores: HOST array of J DEVICE pointers, 0 <= J <= 3, to float32 [N,P] uncertainty maps (entropy, mutual information, anything
 *   where larger means less sure; may be NULL when J == 0); scales: HOST array of J floats, each finite and > 0.
 *   Per pixel, t = lut[gt].  t == 255: the pixel is ignored and counted nowhere.  C <= t < 255: bad[0] += 1 and nothing else.  Otherwise, in fp32,
 *   no product contracted into a sum:
 *     k = argmax_c p_c (the lowest index on ties; c replaces the running maximum only if p_c > it, so a NaN at c > 0 never wins), conf = p_k,
 *     ok = (k == t).  If conf or one of the J scores is NaN or +-inf: bad[1] += 1 and nothing else (the other p_c are not examined).
 *     b = min(B - 1, (int)(conf * (float)B)), 0 for conf < 0;  calib[b] += {1, ok, q_conf},  q_conf = (int64)rintf(conf * 2^24)
 *     sums += {1, ok, q_nll, q_brier},  q_nll = (int64)rintf(-logf(max(p_t, FLT_MIN)) * 2^16),
 *                                       q_brier = (int64)rintf((sum_c (p_c - [c == t])^2, folded in class order from 0) * 2^23)
 *     Score histograms of M = FCN8S_REL_SCORE_BINS bins in ascending uncertainty: score 0 is u = 1 - conf with scale (float)M (the maximum softmax
 *     probability baseline), score j >= 1 is the caller's map j - 1 with scales[j - 1];  for a score s with scale sigma:
 *     bin = s > 0 ? min(M - 1, (int)(s * sigma)) : 0  (a product beyond int's range lands in M - 1);  hist[j][bin][ok ? 0 : 1] += 1.
 *   The fixed point makes every sum an integer (at most 2^-25, 2^-17, 2^-24 of quantisation per pixel) that is the same bits on every run.
 *   calib [B][3], sums [4], hist [1 + J][M][2], bad [2], all int64, are accumulated into, over the N images and over calls (the caller clears
 *   them).  1 <= B <= 64.  Stream-ordered; does not synchronise; allocates nothing; needs no scratch.  FCN8S_ERR_BAD_ARG (nothing launched) for a
 *   NULL prob / gt / lut / table, N or P <= 0, C < 2, B outside 1..64, J outside 0..3, a NULL scores / scales array or score pointer among the J, a
 *   scale that is not finite and > 0; FCN8S_ERR_SHAPE for P >= 2^31.
 *   The kernel takes FCN8S_REL_TILE_PIXELS pixels per block and trip on at most FCN8S_REL_MAX_BLOCKS blocks (more only beyond 2^41 pixels). */
#define FCN8S_REL_SCORE_BINS 1024
#define FCN8S_REL_TILE_PIXELS 256
#define FCN8S_REL_MAX_BLOCKS 1024
int fcn8s_op_reliability_pair(void* stream, const float* prob, const uint8_t* gt, const uint8_t* lut, int N, int64_t P, int C,
                              const float* const* scores, const float* scales, int J, int B,
                              int64_t* calib, int64_t* sums, int64_t* hist, int64_t* bad);
/* Temperature scaling (Guo et al., ICML 2017): the remedy for what fcn8s_op_reliability_pair measures.  One scalar T is fitted on a validation set by
 * minimising the NLL of the calibrated distribution and then applied; the argmax never changes.  The map acts on a distribution, so it applies to
 * whatever a route returns (single pass, multi-scale / flip mean, CRF output).  For beta = 1 / T and a row p of C floats, in fp32 with the natural
 * logarithm, no product contracted into a sum:
 *     l_c = logf(max(p_c, FLT_MIN));   m = max_c l_c;   d_c = l_c - m        (d of the argmax is exactly 0)
 *     e_c = expf(beta * d_c);          s = sum_c e_c   folded in class order from 0   (s >= 1)
 *     q_c = e_c / s                                    the calibrated distribution
 *     nll(beta) = logf(s) - beta * d_t                 (>= 0), t = the true class
 *   For a single-pass softmax this is softmax(z / T) exactly in real arithmetic.  nll is convex in beta, so a bracketing grid search is safe (the
 *   host side of the fit is temperature.py).  The kernels evaluate e_c as v_exp_f32(fl(beta * log2(e)) * d_c); temperature.hip bounds the difference.
 * fcn8s_op_temperature_nll: the objective for K candidates in one pass over a batch of N images of P pixels each on DEVICE pointers.
 *   prob [N,P,C] float32, any C >= 2 and any float alignment; gt [N,P] uint8, any alignment; lut: 256 uint8 on the device; betas: HOST array of K
 *   floats, 1 <= K <= FCN8S_TS_MAX_CANDIDATES, each finite and in [2^-6, 2^6].  Per pixel, t = lut[gt].  t == 255: the pixel is ignored.
 *   C <= t < 255: bad[0] += 1 and nothing else.  Any p_c NaN or +-inf (tested before the clamp): bad[1] += 1 and nothing else.  Otherwise
 *   count += 1 and, for every k, nll[k] += (int64)rintf(nll(beta_k) * 2^16); the l_c and d_c are formed once per pixel for all K candidates.
 *   nll [K], count [1], bad [2], all int64, are accumulated into, over the N images and over calls (the caller clears them).  Integers only: two
 *   runs give the same bits and any partition of the pixels over calls gives the same tables.  Stream-ordered; does not synchronise; allocates
 *   nothing; needs no scratch.  FCN8S_ERR_BAD_ARG (nothing launched) for a NULL pointer, N or P <= 0, C < 2, K outside 1..32, a beta that is not
 *   finite or outside [2^-6, 2^6]; FCN8S_ERR_SHAPE for P >= 2^31.
 * fcn8s_op_temperature_apply: out [N,P,C] (may be NULL; may be prob itself: in place) = q, entropy_out [N,P] (may be NULL) = h(q) =
 *   -sum_c q_c logf(max(q_c, FLT_MIN)) folded in class order (the arithmetic of fcn8s_predict_mc's entropy).  A row that holds a NaN or +-inf
 *   becomes all NaN, with NaN entropy, so that a later fcn8s_op_reliability_pair counts it in bad[1].  beta as above.  Stream-ordered; does not
 *   synchronise; allocates nothing.  FCN8S_ERR_BAD_ARG (nothing launched) for a NULL prob, both outputs NULL, N or P <= 0, C < 2, a beta out of
 *   range; FCN8S_ERR_SHAPE for P >= 2^31.
 *   Both kernels take FCN8S_TS_TILE_PIXELS pixels per block and trip on at most FCN8S_TS_MAX_BLOCKS blocks. */
#define FCN8S_TS_MAX_CANDIDATES 32
#define FCN8S_TS_TILE_PIXELS 256
#define FCN8S_TS_MAX_BLOCKS 1024
int fcn8s_op_temperature_nll(void* stream, const float* prob, const uint8_t* gt, const uint8_t* lut, int N, int64_t P, int C,
                             const float* betas, int K, int64_t* nll, int64_t* count, int64_t* bad);
int fcn8s_op_temperature_apply(void* stream, const float* prob, int N, int64_t P, int C, float beta, float* out, float* entropy_out);
/* Class-balanced pseudo-labels (self-training on hard labels with one confidence threshold per class: CBST, Zou et al., ECCV 2018) from a softmax,
 * for a batch of N images of P pixels each on DEVICE pointers, in one pass that reads every input byte once.  Two uses: the fit sweep
 * (labels_out NULL) fills, per predicted class, a histogram of the maximum softmax probability, from which the host takes the thresholds
 * (pseudo_label.py); the export sweep writes label maps that hold the class where it clears its threshold and ignore_id elsewhere.
 *   prob [N,P,C] float32, as fcn8s_predict (argmax = 0), fcn8s_predict_tta, fcn8s_predict_crf and fcn8s_predict_mc write it; any 2 <= C <= 255 and
 *   any float alignment (16-byte loads are used when the pointer is 16-byte aligned and C % 4 == 0).  thresholds: float32[C], may be NULL: every
 *   threshold is 0.  out_ids: uint8[C], the label written for class k, may be NULL: k itself.  ignore_id (0..255): written where a pixel is not
 *   kept.  base [N,P] uint8 or NULL: existing labels, with base_fill (0..255) marking the pixels to fill.  score [N,P] float32 or NULL: an
 *   uncertainty map, gated at score_max (finite).  labels_out [N,P] uint8, any alignment; may be NULL: tables only.
 *   Tables, all int64, accumulated into, over the N images and over calls (the caller clears them): hist [C][M], M = FCN8S_PL_BINS (may be
 *   NULL); counts [C][2] = {kept, dropped}; misc [3] = {bad rows, passed-through base pixels, dropped by score}.
 *   Per pixel p, in this order, in fp32, nothing contracted:
 *     1. base given and base[p] != base_fill: labels_out[p] = base[p], misc[1] += 1, and nothing else (the row is not examined).
 *     2. k = argmax_c p_c (the lowest index on ties; c replaces the running maximum only if p_c > it, so a NaN at c > 0 never wins), conf = p_k.
 *        conf NaN or +-inf: misc[0] += 1, the label is ignore_id, and nothing else.
 *     3. score given and not (score[p] <= score_max) (a NaN score fails): misc[2] += 1, counts[k][1] += 1, the label is ignore_id; the pixel
 *        does not enter hist.
 *     4. b = conf > 0 ? min(M - 1, (int)(conf * (float)M)) : 0;  hist[k][b] += 1.
 *     5. conf >= thresholds[k]: the label is out_ids[k] and counts[k][0] += 1; otherwise the label is ignore_id and counts[k][1] += 1.
 *   M is a power of two, so conf * M is exact, and for a threshold on a bin edge j / M: conf >= j / M <=> b >= j for every conf in [0, 1).  With
 *   edge thresholds the kept count of class k in a second sweep therefore equals the tail sum of hist[k][j ..] of the first, exactly.
 *   Integers only decide the tables: two runs give the same bits, and so does any partition of the pixels over calls.  Stream-ordered; does not
 *   synchronise; allocates nothing; needs no scratch.  FCN8S_ERR_BAD_ARG (nothing launched) for a NULL prob / counts / misc, labels_out and hist
 *   both NULL, N or P <= 0, C outside 2..255, ignore_id or base_fill outside 0..255, base without labels_out, a score_max that is not finite;
 *   FCN8S_ERR_SHAPE for P >= 2^31.
 *   The kernel takes FCN8S_PL_TILE_PIXELS pixels per block and trip on at most FCN8S_PL_MAX_BLOCKS blocks (more only beyond 2^40 pixels). */
#define FCN8S_PL_BINS 1024
#define FCN8S_PL_TILE_PIXELS 256
#define FCN8S_PL_MAX_BLOCKS 512
int fcn8s_op_pseudo_label(void* stream, const float* prob, int N, int64_t P, int C, const float* thresholds, const uint8_t* out_ids, int ignore_id,
                          const uint8_t* base, int base_fill, const float* score, float score_max, uint8_t* labels_out,
                          int64_t* hist, int64_t* counts, int64_t* misc);
/* ClassMix (Olsson et al., WACV 2021; the mixing of DACS, Tranheden et al., WACV 2021) for a batch of N images of P pixels each on DEVICE
 * pointers: half of the classes present in a source image are cut out along its label mask and pasted onto a destination image, pixels and
 * labels alike.  Integers only.
 *   images [N,P,3] uint8, labels [N,P] uint8 (ids >= C, the ignore id among them, are not classes), src [N] int32 on the device: the source
 *   image of destination n.  2 <= C <= 255.  For destination n with source s = src[n]:
 *   1. Presence.  Class c < C is present in s when at least one pixel of labels[s] equals c; k = the number of present classes.
 *   2. Selection.  key(c) = philox_u32(draw * 2^16 + n * 2^8 + c, seed, 0x434D4958), the library's counter-based generator (ten Philox-4x32
 *      rounds; the dropout masks use the same).  rank(c) = the number of present c' with (key(c'), c') < (key(c), c), compared lexicographically.
 *      c is selected iff it is present and rank(c) < m, m = ceil(k / 2) (ClassMix's count); k = 0 selects nothing.  selected_out [N][256] uint8
 *      (may be NULL) holds 1 or 0 per class, 0 for every c >= C.
 *   3. Mix.  Where labels[s][p] < C and that class is selected: out_images[n][p][:] = images[s][p][:] and out_labels[n][p] = labels[s][p];
 *      elsewhere both come from image n.  src[n] == n is legal and yields image n.
 *   A src[n] outside [0, N) cannot be refused on the host: the kernels treat it as n and set a flag.
 * work: fcn8s_op_class_mix_work_bytes(N) bytes of device scratch at any alignment, whose content on entry does not matter.  Behind its first
 * 16-byte boundary b it holds the presence sets (32 N bytes), the tables (256 N bytes) and, at b + 288 N, the flag: a uint32 that is 0 after a
 * call whose src was in range and 1 otherwise.
 * Any byte alignment of every pointer: every stream moves as 16-byte accesses of whole lines of memory, byte by byte at its ragged ends; no byte
 * outside the outputs is written.  The outputs must not overlap the inputs.  Only integer ORs and compares decide anything: two runs give the same
 * bits.  Stream-ordered; does not synchronise; allocates nothing.  FCN8S_ERR_BAD_ARG (nothing launched, the outputs untouched) for a NULL images /
 * labels / src / work / out_images / out_labels, N or P <= 0, C outside 2..255, draw >= 2^48, an output range that overlaps images, labels or
 * src; FCN8S_ERR_SHAPE for N > 256 or P >= 2^31. */
size_t fcn8s_op_class_mix_work_bytes(int N);
int fcn8s_op_class_mix(void* stream, const uint8_t* images, const uint8_t* labels, const int32_t* src, int N, int64_t P, int C, uint64_t seed,
                       uint64_t draw, void* work, uint8_t* out_images, uint8_t* out_labels, uint8_t* selected_out);
/* Strong photometric augmentation of a batch of N uint8 RGB images of H x W pixels on DEVICE pointers -- the colour jitter and Gaussian blur that
 * DACS (Tranheden et al., WACV 2021) and ClassMix (Olsson et al., WACV 2021) apply to the student's input and not to the labeler's.  Integers plus
 * the float32 steps of the 8-bit HSV -> RGB conversion of fcn8s_op_augment_u8 (OpenCV's RGB2HSV_b / HSV2RGB_b, H in [0, 180)).
 *   images, out_images [N,H,W,3] uint8 on the device, at any byte alignment; they must not overlap (the blur reads neighbours).
 *   jitter, blur and taps are HOST pointers, read before the call returns and passed to the kernels by value (no device table, no upload):
 *   jitter = {gate, Cs, Ss, Bs, Hs} int32, NULL = no colour step; blur = {gate, Q, R} int32 with taps [Q][R + 1] uint16, both NULL = no blur.
 *   Gates lie in 0..65536 (65536 = always), 0 <= Cs, Ss, Bs <= 65536, 0 <= Hs <= 90, 1 <= Q <= 16, 1 <= R <= 7; every row w of taps has
 *   w[0] + 2 (w[1] + ... + w[R]) = 2048 and w[i] <= w[i - 1].
 *   Draws.  u_j = philox_u32(draw * 2^16 + n * 2^8 + j, seed, 0x53415547) for j = 0..6: the library's generator on a stream of its own, with
 *   fcn8s_op_class_mix's counters, so that one (seed, draw) serves both.  U(u, S) = -S + ((u (2 S + 1)) >> 32) in 64 bits: uniform in [-S, S].
 *   Colour step, for image n iff (u_0 >> 16) < gate:
 *   1. Contrast, only when Cs != 0: c16 = 65536 + U(u_1, Cs); m = (2 G + P) / (2 P) in integers, P = H W, G = the sum over the INPUT image of
 *      g = (4899 R + 9617 G + 1868 B + 8192) >> 14; per channel t = x c16 + m (65536 - c16) + 32768 (signed 32 bits), x' = clamp(t >> 16, 0, 255)
 *      with an arithmetic shift.
 *   2. HSV, only when Ss | Bs | Hs != 0: (H, S, V) = RGB2HSV_b(x'); H' = (H + 180 + U(u_4, Hs)) mod 180; S' = min(255, (S s16 + 32768) >> 16) with
 *      s16 = 65536 + U(u_2, Ss); V' likewise with b16 = 65536 + U(u_3, Bs); x'' = HSV2RGB_b(H', S', V').  All strengths 0 leave every byte as it is.
 *   Blur, for image n iff (u_5 >> 16) < blur gate, of the colour step's output: q = (u_6 Q) >> 32, w = taps[q]; separable, per channel, borders
 *   reflect-101 (index -i reads i, W - 1 + i reads W - 1 - i); a = sum_i w[|i|] x[. + i] along the row, b = sum_i w[|i|] a[. + i] down the column
 *   (b <= 255 * 2^22), out = (b + 2^21) >> 22: no intermediate rounding.  An image whose gates both fail is copied.
 *   params_out [N][8] int32 on the device (may be NULL): per image {colour step ran, c16, s16, b16, dh, m, blur ran, q}, 0 for what did not run
 *   (c16 and m without contrast, s16, b16 and dh without the HSV step, q without the blur).
 * work: fcn8s_op_strong_augment_work_bytes(N) bytes of device scratch at any alignment, whose content on entry does not matter; it holds the N
 * 64-bit grey sums at its first 16-byte boundary.  The sums are integer adds (one 64-bit atomic per block): two runs give the same bits.
 * Stream-ordered; does not synchronise; allocates nothing.  No byte outside out_images is written.
 * FCN8S_ERR_BAD_ARG (nothing launched, the outputs untouched) for a NULL images / work / out_images, N, H or W <= 0, draw >= 2^48, a gate or a
 * strength out of range, Q outside 1..16, R outside 1..7, taps NULL when blur is not, a row of taps that does not sum to 2048 or increases,
 * out_images overlapping images; FCN8S_ERR_SHAPE for N > 256, H W >= 2^31, or H <= R or W <= R when blur is not NULL (one reflection suffices). */
size_t fcn8s_op_strong_augment_work_bytes(int N);
int fcn8s_op_strong_augment(void* stream, const uint8_t* images, int N, int H, int W, uint64_t seed, uint64_t draw, const int32_t* jitter,
                            const int32_t* blur, const uint16_t* taps, void* work, uint8_t* out_images, int32_t* params_out);
/* Fourier domain adaptation (FDA: Yang & Soatto, CVPR 2020) of a batch of N source images towards M target images, uint8 RGB of the same H x W on
 * DEVICE pointers: the amplitudes of the (2 b + 1)^2 lowest frequencies of every source image become those of its target image, the phases stay.
 *   images [N,H,W,3], targets [M,H,W,3] uint8; pair_dev [N] int32 on the device, pair[n] in [0, M) the target of source n (NULL: n mod M);
 *   b the half-width, 0 <= b <= 96 and B = 2 b + 1 <= min(H, W) (beta <= 0.09 up to a short side of 1024; the window never wraps onto itself).
 *   Per source n, target t = pair[n] and channel, for u, v in {-b .. b}:
 *     F_s(u,v) = sum_h sum_w x_s[h,w] exp(-2 pi i (u h / H + v w / W)),  F_t likewise from x_t
 *     A_s = |F_s|, A_t = |F_t|, phi = F_s / A_s (phi = 1 where A_s = 0: numpy's angle(0) = 0)
 *     Delta(u,v) = phi (A_t - A_s)
 *     y[h,w] = x_s[h,w] + 1 / (H W) Re sum_u sum_v Delta(u,v) exp(+2 pi i (u h / H + v w / W))
 *     out_f32 = y, out_u8 = clamp(rintf(y), 0, 255)
 *   which equals the published fft2 / fftshift / window [c - b : c + b + 1] / ifftshift / ifft2 route (c = floor(H / 2), floor(W / 2)); the published
 *   code does not clip, it trains on floats.  Four rules belong to the definition:
 *   1. Twiddles.  Every exp(+-2 pi i k / n) comes from the integer-reduced phase (f index) mod n (here: a table of sincospi(2 k / n), k < n).
 *   2. Equal spectra cancel exactly.  F_s and F_t come from one instruction sequence, so a source whose target holds the same bytes has
 *      A_t - A_s = 0 exactly: out_u8 == x_s and out_f32 == float(x_s) with ==.
 *   3. Fixed order, batch independence.  No float atomics; every sum is taken in a fixed order; the bits of an image's output depend on that image,
 *      its target, H, W and b only -- not on N, M, the image's place in the batch or what work held on entry.
 *   4. The ill-conditioned case.  Where A_s lies below the rounding of its own sum (a constant source at b >= 1) the phase is noise, as it is in the
 *      published float64 code; such outputs are finite, no more.
 *   The implementation uses F(-u,-v) = conj F(u,v) of a real image: it computes the columns v = 0 .. b and takes the other half of the window as
 *   their conjugates.  The two large products (rows of an image against the W twiddles, both ways) are float32 v_mfma_f32_32x32x2_f32 chains, the
 *   sum over h and Delta are double, the sum over u is a float32 fmaf chain.
 * work: fcn8s_op_fda_work_bytes(N, M, H, W, b) bytes of device scratch at any alignment, whose content on entry does not matter (the twiddle tables
 * are rebuilt by a small kernel in every call).  At its first 16-byte boundary it holds the flag: a uint32 that is 0 after a call whose pair_dev
 * was in range and 1 otherwise -- a pair_dev[n] outside [0, M) lives on the device, cannot be refused, and counts as n mod M.
 * images, targets and out_u8 at any byte alignment (16-byte accesses of whole lines, byte by byte at the ragged ends), out_f32 4-byte aligned;
 * one of the two outputs may be NULL; no byte outside the outputs is written; the outputs must not overlap the inputs, work or each other.
 * Stream-ordered; does not synchronise; allocates nothing.  FCN8S_ERR_BAD_ARG (nothing launched, the outputs untouched) for a NULL images / targets /
 * work, both outputs NULL, N, M, H or W <= 0, b < 0, b > 96, 2 b + 1 > min(H, W), a misaligned out_f32, an overlap; FCN8S_ERR_SHAPE for N or M > 256
 * or H W >= 2^31. */
size_t fcn8s_op_fda_work_bytes(int N, int M, int H, int W, int b);
int fcn8s_op_fda_transfer(void* stream, const uint8_t* images, int N, const uint8_t* targets, int M, int H, int W, int b, const int32_t* pair_dev,
                          void* work, uint8_t* out_u8, float* out_f32);
/* Boundary measures of a segmentation against its ground truth -- the counting half of the trimap IoU (accuracy inside a band of width r around
 * the ground-truth boundaries: Kraehenbuehl & Koltun 2011, Chen et al. 2015) and of the boundary F-score (Csurka et al., BMVC 2013) -- for a batch
 * of N images of H x W pixels on DEVICE pointers.  All integers.
 *   Per image: G = gt_label_ids (uint8 label ids 0..33), P = the predicted label ids (pred_kind 0: int64 train ids 0..19 through the same
 *   trainId -> id table as fcn8s_op_cityscapes_pair; pred_kind 1: uint8 label ids 0..33).  R = the largest radius, 1 <= R <= 16.  Pixels outside
 *   the image do not exist (the image edge is not a boundary).  Distances are squared Euclidean pixel distances dy^2 + dx^2.  The ring of a
 *   squared distance d2 is the smallest integer k >= 0 with k^2 >= d2; if that is larger than R, or nothing was found within R, the ring is R + 1.
 *   1. Trimap rings.  For pixel p, d2(p) = min over q != p with G[q] != G[p] of |q - p|^2; rings[ring(d2(p)) - 1][G[p]][P[p]] += 1.
 *      rings is [R + 1][34][34] int64; index R (ring R + 1) holds the pixels farther than R from every other label.  The band of width r <= R is the
 *      sum of the first r matrices; the sum of all R + 1 is the confusion matrix fcn8s_op_cityscapes_pair counts on the same pixels.  Raw label
 *      ids are compared (a boundary towards an ignored label is a boundary).
 *   2. Boundary sets.  For a map M, B(M) = the pixels that have a 4-neighbour inside the image with another value of M.
 *   3. Boundary precision / recall counts.  For every p in B(P) with c = P[p]: e2(p) = min over q in B(G) with G[q] == c (q = p allowed, distance
 *      0) of |q - p|^2; bprec[ring(e2(p))][c] += 1.  Symmetrically for every p in B(G) with c = G[p] against q in B(P) with P[q] == c:
 *      brec[ring][c] += 1.  Both [R + 2][34] int64; ring 0 = coincident, ring R + 1 = unmatched within R.
 *   4. An id out of range (gt > 33, train id outside 0..19, label id > 33) takes part in every comparison of its map as the id 255 (so it is a
 *      boundary towards every valid neighbour and matches no class); a pixel whose own G or P id is out of range is counted in bad[0] and in none
 *      of the three tables.  The Python layer refuses an image with bad != 0.
 *   rings, bprec, brec and bad are accumulated into, over the N images and over calls (the caller clears them).  Integers only: two runs give the
 *   same bits.  Any H, W and alignment.  Stream-ordered; does not synchronise; allocates nothing.  FCN8S_ERR_BAD_ARG (nothing launched) for a NULL
 *   pointer, pred_kind outside {0, 1}, N, H or W <= 0, R outside 1..16; FCN8S_ERR_SHAPE for H * W >= 2^31.
 *   Host side (cityscapes_eval.py): trimap IoU of width r = the evaluator's IoU on the summed first r matrices; boundary precision of class c at
 *   tolerance t = sum(bprec[0..t][c]) / sum(bprec[:][c]), recall likewise from brec, F = 2 P R / (P + R). */
int fcn8s_op_boundary_pair(void* stream, const uint8_t* gt_label_ids, const void* pred, int pred_kind, int N, int H, int W, int R,
                           int64_t* rings, int64_t* bprec, int64_t* brec, int64_t* bad);
/* The distance map of the boundary-weighted cross-entropy (defined at fcn8s_op_softmax_xent_px) for a batch of N label maps of H x W pixels on
 * DEVICE pointers:
 * codes_out[n][y][x] = d2 if d2 <= R^2, else 255.  uint8 in, uint8 out; integers only: two runs give the same bits.  Any H, W and alignment of
 * either pointer.  Stream-ordered; does not synchronise; allocates nothing.  FCN8S_ERR_BAD_ARG (nothing launched) for a NULL pointer, N, H or
 * W <= 0, or R outside 1..15; FCN8S_ERR_SHAPE for H * W >= 2^31. */
int fcn8s_op_boundary_distance(void* stream, const uint8_t* label_ids, int N, int H, int W, int R, uint8_t* codes_out);
/* Connected regions of a label map, and the cleanup of small ones (the usual post-processing of an argmax map: the specks inside a car or on a
 * wall are merged into a neighbour), for a batch of N maps of H x W pixels on DEVICE pointers.  All integers.
 *   Per image: a label map L[H, W] of class ids 0..255, pixel index i = y * W + x.  labels [N,H,W]: label_kind 0 = int64 as fcn8s_predict writes
 *   it (read as 16-byte loads where the address allows), 1 = uint8 (any alignment, any W).  connectivity is 4 or 8.
 *   Components.  A component is a maximal set of pixels of equal class connected under `connectivity`.  Its id is the smallest pixel index it
 *   contains; ids are per image (not offset by n * H * W) and depend on nothing but the map.  comp[p] = the id of p's component, area[p] = the
 *   number of pixels of p's component, both int32 [N,H,W], both stored at every pixel.
 *   Small.  A component of class c is small when area < min_area[c]; min_area[c] <= 0: class c is never small.  min_area: 256 int32 on the device.
 *   One round of cleanup.  For a small component S look at every pair (p in S, q 4-adjacent to p, q not in S) -- 4-adjacent under either
 *   connectivity.  Only a q whose component T is not small is a candidate.  S takes the class of the candidate T with the largest area, the
 *   smaller id on equal areas (the label found at pixel id(T)); without a candidate S keeps its class.  All decisions of a round are taken on that
 *   round's input map and applied together.  `rounds` rounds (1..8) run back to back, each on the components of the previous round's output.
 *   stats (may be NULL) [rounds][4] int64, written, not accumulated: components, small components, relabelled components, pixels changed.
 *   A label outside 0..255 in an int64 map is the caller's error; such a pixel is a component of its own (area 1) that is never small, is no
 *   candidate, and is never written; the pixels of this kind met by the call are counted in the work header (fcn8s_op_regions_status).
 * fcn8s_op_regions_label writes comp_out and, unless it is NULL, area_out.  fcn8s_op_regions_clean rewrites labels in place.
 * work: fcn8s_op_regions_work_bytes(N, H, W) bytes of 16-byte aligned device scratch = a header of 8192 bytes + 16 bytes per pixel (label uses the
 * first 256 bytes alone);
 * its content on entry does not matter, and a buffer that is large enough may be reused for any shape.
 * Both are a block-based union-find in which only integer min / max / add atomics decide anything: two runs give the same bits.  Every loop is
 * bounded: a find follows strictly decreasing indices, a union gives up after a fixed number of retries; a loop that meets what cannot be
 * (never seen) sets a bit in the work header instead of spinning.  fcn8s_op_regions_status synchronises the stream and copies {those bits (0 = sound),
 * pixels with a label out of range} of the most recent label / clean call on `work` into status_host[2].
 * label and clean are stream-ordered, do not synchronise and allocate nothing.  FCN8S_ERR_BAD_ARG (nothing launched) for a NULL labels / comp_out /
 * min_area / work, a work that is not 16-byte aligned, label_kind outside {0, 1}, connectivity outside {4, 8}, rounds outside 1..8, N, H or W <= 0;
 * FCN8S_ERR_SHAPE for H * W >= 2^31 or N > 65535. */
size_t fcn8s_op_regions_work_bytes(int N, int H, int W);
int fcn8s_op_regions_label(void* stream, const void* labels, int label_kind, int N, int H, int W, int connectivity,
                           int32_t* comp_out, int32_t* area_out, void* work);
int fcn8s_op_regions_clean(void* stream, void* labels, int label_kind, int N, int H, int W, int connectivity,
                           const int32_t* min_area_dev, int rounds, void* work, int64_t* stats_dev);
int fcn8s_op_regions_status(void* stream, const void* work, int64_t* status_host);
/* The counting half of panoptic quality (PQ = SQ x RQ: Kirillov et al., CVPR 2019; reported by the Cityscapes benchmark since 2019) for a batch of N
 * images of H x W pixels on DEVICE pointers: per image the sparse joint table "pixels shared by predicted segment kp and ground-truth segment kg".
 * All integers.  Train ids are those of labels.py as modified by the reference's author: 0 = void, 1..11 = stuff, 12..19 = things (the labels that
 * have instances and are evaluated: person .. bicycle).
 *   Predicted segments, from the argmax a[p] (pred_kind 0: int64 train ids 0..19 as fcn8s_predict writes them; pred_kind 1: uint8 label ids 0..33,
 *   mapped to train ids first -- labels.py id -> trainId) and pred_comp[p] = comp_out of fcn8s_op_regions_label on the same map (connectivity 4 or 8
 *   is the caller's choice there):
 *     a = 0 (void): no segment, kp = 0;  stuff class c: one segment per image, kp = c;
 *     thing class c: one segment per connected component, kp = 2^31 | comp << 5 | c   (hence H * W <= 2^26).
 *     A prediction outside 0..19 (a label id outside 0..33) is counted as bad and the pixel is skipped.
 *   Ground-truth segments, from the instance map alone (uint16, *_gtFine_instanceIds.png), as the official panoptic conversion does.  For the
 *   value v: L = v if v < 1000 else v / 1000, t = trainId(L).
 *     t = 0 (void or ignoreInEval): kg = 0;  L > 33: the pixel is counted as bad and skipped;  stuff: kg = t;
 *     a thing with v >= 1000: kg = 2^31 | (v % 1000) << 5 | t;   a thing with v < 1000 is a crowd region, one per class: kg = 2^30 | t.
 *   The table of an image holds every distinct (kp, kg) with its pixel count, void on either side included: the counts sum to H * W minus the
 *   bad pixels.
 *   rows [N][max_rows][3] int64 = {kp, kg, pixels} of image n, in no particular order (callers sort); counts [N][4] int64, written, not
 *   accumulated = {rows found -- it may exceed max_rows, then only max_rows rows were written and the call is to be repeated with more room --,
 *   bad pixels, 1 if the hash table was too small (then the rows are to be discarded and the call repeated with more slots), pixels counted}.
 *   work: fcn8s_op_panoptic_work_bytes(N, slots_per_image) bytes of 16-byte aligned device scratch = 16 bytes per slot (0 for a slot count that
 *   is refused); its content on entry does not matter.  slots_per_image: a power of two in 1 .. 2^28; a table of at least 2 H W slots cannot
 *   be too small.  Any pointer alignment of the three maps (16-byte loads where the address allows, scalar loads otherwise).
 *   Scores (panoptic.py; float64 on the host, rows in ascending (kp, kg) order, images in file order).  Segment areas are the marginals of the
 *   table.  A row with kp != 0, kg != 0, kg no crowd region and equal classes has iou = n / (area_p + area_g - n - count(kp, 0)); iou > 0.5 is a
 *   match: tp[c] += 1, iou_sum[c] += iou.  An unmatched ground-truth segment that is no crowd region: fn[c] += 1.  An unmatched predicted
 *   segment: fp[c] += 1, unless (count(kp, 0) + count(kp, crowd of c)) / area_p > 0.5.  Per class PQ = iou_sum / (tp + fp / 2 + fn / 2),
 *   SQ = iou_sum / tp (0 when tp = 0), RQ = tp / (tp + fp / 2 + fn / 2); averages over the classes with tp + fp + fn > 0.
 *   Connected components are the naive way to turn a semantic map into instances (touching cars are one segment): PQ of the things measures
 *   the semantic model plus that rule; PQ of the stuff classes and the fp counts are what the table is for.
 * Only compare-and-swap on a slot's key and integer adds on its count decide anything: two runs give the same set of rows.  No kernel waits
 * for another block and every probe loop is bounded.  Stream-ordered; does not synchronise; allocates nothing.  FCN8S_ERR_BAD_ARG (nothing
 * launched) for a NULL pointer, a work that is not 16-byte aligned, pred_kind outside {0, 1}, N, H or W <= 0, max_rows < 1, slots_per_image no
 * power of two in 1 .. 2^28; FCN8S_ERR_SHAPE for H * W > 2^26 or N > 65535. */
size_t fcn8s_op_panoptic_work_bytes(int N, int64_t slots_per_image);
int fcn8s_op_panoptic_pair(void* stream, const uint16_t* gt_instance_ids, const void* pred, int pred_kind, const int32_t* pred_comp, int N, int H, int W,
                           void* work, int64_t slots_per_image, int64_t* rows, int64_t max_rows, int64_t* counts);
/* The counting half of instance-level AP (the Cityscapes instance-level evaluation: AP over the overlaps 0.5 .. 0.95 and AP50% per thing class) for
 * a batch of N images of H x W pixels on DEVICE pointers: per image the sparse joint table "pixels shared by predicted instance kp and ground-truth
 * instance value v", with the summed confidence of those pixels.  Train ids as above: 0 = void, 1..11 = stuff, 12..19 = things.  C >= 20.
 *   Inputs per pixel p: labels[p], a uint8 train id -- the class the pixel ended up with: the argmax of the softmax, possibly after
 *   fcn8s_op_regions_clean; comp[p] = comp_out of fcn8s_op_regions_label on that same map; prob [N,H*W,C] float32 as fcn8s_predict (argmax = 0)
 *   and its siblings write it; v[p] = gt_instance_ids[p] (uint16, *_gtFine_instanceIds.png), 0 when the pointer is NULL (the export route).
 *   Predicted key.  labels[p] in 12..19: kp = 2^31 | comp << 5 | labels[p], the thing key of fcn8s_op_panoptic_pair (hence H * W <= 2^26).  Otherwise
 *   kp = 0, "no instance"; a label >= 20 also gives kp = 0 and is counted as bad.
 *   Ground-truth key.  The raw value v and nothing else -- not fcn8s_op_panoptic_pair's kg, which sends every ignoreInEval label to 0: the
 *   instance-level evaluation does not (a caravan instance 29001 is neither void nor a match; only values that equal an ignored label id,
 *   v < 1000, are void).  The raw value lets the host apply those rules exactly.
 *   Confidence.  Where kp != 0: q = prob[p][labels[p]], the probability of the assigned class (which also holds after a cleanup), and the term
 *   t = (int64)rintf(q * 2^24), the fixed point of fcn8s_op_reliability_pair.  A q that is not in [0, 1] (NaN fails the test) gives t = 0 and is
 *   counted.  Where kp = 0 the row is not examined and t = 0.
 *   The table of an image holds every distinct (kp, v), kp = 0 included, with n = its pixel count and s = the sum of its terms: the counts sum
 *   to H * W.  n <= 2^26 and t <= 2^24, so s < 2^51.
 *   rows [N][max_rows][4] int64 = {kp, v, n, s} of image n, in no particular order (callers sort); counts [N][5] int64, written, not accumulated
 *   = {rows found -- it may exceed max_rows, then only max_rows rows were written and the call is to be repeated with more room --, pixels with a
 *   label >= 20, 1 if the hash table was too small (then the rows are to be discarded and the call repeated with more slots), pixels counted,
 *   pixels with q out of range}.
 *   work: fcn8s_op_instance_work_bytes(N, slots_per_image) bytes of 16-byte aligned device scratch = 32 bytes per slot (0 for a slot count that
 *   is refused); its content on entry does not matter.  slots_per_image: a power of two in 1 .. 2^28; a table of at least 2 H W slots cannot
 *   be too small.  Any byte alignment of the three maps and any float alignment of prob (16-byte loads of the rows when prob is 16-byte
 *   aligned and C % 4 == 0, 4-byte loads otherwise).
 *   Host half (instances.py; float64).  Area of a predicted instance = sum_v n; confidence = sum_v s / (area * 2^24); void intersection = sum of
 *   n over the void v (v < 1000 whose label is ignored in the evaluation); intersection with a ground-truth instance = n(kp, v) for the v
 *   whose label (v if v < 1000, else v / 1000) is the instance's class; ground-truth pixel count of v = sum_kp n (which is why kp = 0 is in the
 *   table); v / 1000 > 33 is refused for the image.  Then the matching and the curve of the Cityscapes instance-level evaluation: overlaps
 *   0.5 .. 0.95 in steps of 0.05; ground-truth regions below 100 pixels and group regions (v < 1000 of the class) are ignore regions; a prediction
 *   without a match is dropped when its ignored share exceeds the overlap threshold; hard false negatives are counted; AP is the step-wise
 *   integral of the precision-recall curve; averages are NaN-skipping means over the classes.  The distance-based variants are not taken.
 *   Connected components are the naive way to turn a semantic map into instances (touching cars are one instance): AP under this rule measures
 *   the semantic model plus that rule -- a baseline and a speck detector, not an instance-segmentation method.
 * Only compare-and-swap on a slot's key and integer adds on its count and sum decide anything: two runs give the same set of rows.  No kernel
 * waits for another block and every probe loop is bounded.  Stream-ordered; does not synchronise; allocates nothing.  FCN8S_ERR_BAD_ARG (nothing
 * launched, outputs untouched) for a NULL prob / labels / comp / work / rows / counts, a work that is not 16-byte aligned, a prob that is not
 * 4-byte aligned, C < 20, N, H or W <= 0, max_rows < 1, slots_per_image no power of two in 1 .. 2^28; FCN8S_ERR_SHAPE for H * W > 2^26,
 * N > 65535 or C > 2^18. */
size_t fcn8s_op_instance_work_bytes(int N, int64_t slots_per_image);
int fcn8s_op_instance_pair(void* stream, const float* prob, int C, const uint8_t* labels, const int32_t* comp,
                           const uint16_t* gt_instance_ids /* may be NULL */, int N, int H, int W,
                           void* work, int64_t slots_per_image, int64_t* rows, int64_t max_rows, int64_t* counts);
/* One TF-Adam (step t, 1-based) / SGD-momentum step over n floats on DEVICE pointers, the gradient scaled by grad_scale.  Every pointer may
 * have any float (4-byte) alignment of its own.  These two, their _dev and their _ema forms below run one kernel and give the same bits. */
int fcn8s_op_tf_adam(void* stream, float* theta, const float* g, float* m, float* v, int64_t n, int t,
                     float lr, float beta1, float beta2, float eps, float grad_scale);
int fcn8s_op_sgd_momentum(void* stream, float* theta, const float* g, float* buf, int64_t n,
                          float lr, float momentum, float grad_scale);
/* the kernels of fcn8s_accumulate_bucket and of the clipped update on DEVICE pointers of any float alignment.  grad_accumulate: mode 0:
 * dst = src, 1: dst = dst + src, n floats.  grad_norm: out5_dev = float[5] {norm, c, s, ok (1 / 0), 0} of the n floats at g as defined at
 * fcn8s_set_grad_clip (max_norm = 0: c = 1); it allocates its slab of partial sums and synchronises.  tf_adam_dev / sgd_momentum_dev:
 * fcn8s_op_tf_adam / fcn8s_op_sgd_momentum with grad_scale = out5_dev[2], at any float alignment like them; out5_dev[3] == 0: nothing is touched. */
int fcn8s_op_grad_accumulate(void* stream, float* dst, const float* src, int64_t n, int mode);
int fcn8s_op_grad_norm(void* stream, const float* g, int64_t n, float grad_scale, float max_norm, float* out5_dev);
int fcn8s_op_tf_adam_dev(void* stream, float* theta, const float* g, float* m, float* v, int64_t n, int t,
                         float lr, float beta1, float beta2, float eps, const float* out5_dev);
int fcn8s_op_sgd_momentum_dev(void* stream, float* theta, const float* g, float* buf, int64_t n,
                              float lr, float momentum, const float* out5_dev);
/* the kernels of "the average" on DEVICE pointers of any float alignment.  ema_update: s <- s - w (s - theta) over n floats, w =
 * one_minus_decay; out5_dev (may be NULL) is a slab as fcn8s_op_grad_norm writes it: out5_dev[3] == 0 touches nothing.  tf_adam_ema /
 * sgd_momentum_ema: fcn8s_op_tf_adam / fcn8s_op_sgd_momentum (out5_dev == NULL: host grad_scale) or their _dev forms (out5_dev != NULL:
 * grad_scale is ignored) on theta and the slots -- the same bits --, then ema_update of s with the new theta, in one pass.  swap: the n floats
 * at a and at b change places (the ranges must not overlap).  FCN8S_ERR_BAD_ARG for a null pointer or n < 0. */
int fcn8s_op_ema_update(void* stream, float* s, const float* theta, int64_t n, float one_minus_decay, const float* out5_dev);
int fcn8s_op_tf_adam_ema(void* stream, float* theta, const float* g, float* m, float* v, float* s, int64_t n, int t,
                         float lr, float beta1, float beta2, float eps, float grad_scale, const float* out5_dev, float one_minus_decay);
int fcn8s_op_sgd_momentum_ema(void* stream, float* theta, const float* g, float* buf, float* s, int64_t n,
                              float lr, float momentum, float grad_scale, const float* out5_dev, float one_minus_decay);
int fcn8s_op_swap(void* stream, float* a, float* b, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* FCN8S_HIP_H */
