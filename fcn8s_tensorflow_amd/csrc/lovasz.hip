// Lovász-softmax training loss (fcn8s_set_lovasz, fcn8s_op_lovasz_softmax; the definition is in include/fcn8s_hip.h).
//
// Keys and payloads live in a fixed [segment][class][pixel] layout, so the initial order of every segment-class is pixel order and a
// stable LSD radix sort gives the tie rule (e descending, ties by ascending pixel) for free.
//   key     = 0x3F800000 - bits(e) (ascending for descending e, e in [0, 1]); an ignored pixel gets 0x3F800001 and sorts last
//   payload = the pixel's index inside its segment | (foreground << 31)
// Stages, all stream-ordered, no host round trip:
//   1. lov_key_kernel      keys + payloads of every masked class, integer counts G[s][c] (foreground) and V[s] (valid pixels)
//   2. lov_prep_kernel     participation (mask, and G > 0 in `present` mode) -> w[s][c] = 1 / (|S| |C_s|), 0 = not participating
//   3. three 10-bit passes: lov_hist_kernel (per-tile LDS histograms), lov_scan_kernel (per segment-class exclusive scan over
//      (digit, tile)), lov_scatter_kernel (stable in-tile scatter: wave peers by ballots, earlier waves' counts through LDS)
//   4. lov_fgcount_kernel + lov_grad_kernel: the two-level scan of the foreground bits, I_r, U_r and g_r in double from the exact
//      counts, the loss partials e g per tile (tree inside the tile), and the [class][pixel] gradient plane d L / d prob
//   5. lov_finalize_kernel: per segment-class the tiles summed in order (double), the segment means, the batch mean
//   6. lov_bwd_kernel: the softmax recomputed, dlogits += lambda prob (q - <q, prob>), per-block column sums summed in order
// Every sum is integer or in a fixed order: the path is deterministic and has no float atomics.  Non-participating segment-classes
// (w == 0) return at once from every sort kernel; `present` mode reads G from device memory for that.
#include "fcn8s_internal.h"
#include "loss_tile.h"

namespace fcn8s {
namespace {

constexpr int LOV_BITS = 10, LOV_BINS = 1 << LOV_BITS, LOV_IPT = 64, LOV_TILE = 256 * LOV_IPT;   // 16384 keys per tile
constexpr unsigned LOV_IGNORE_KEY = 0x3F800001u;

static __device__ __forceinline__ double lov_block_sum(double v, double* sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = 0;
    if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    __syncthreads();
    return t;   // valid in thread 0
}

// the pixel's probabilities, bit for bit those of softmax_argmax_kernel(_c): prob_c = expf(z_c - max) / sum, classes summed in order
template <int CM>
static __device__ __forceinline__ void lov_probs(const float* x, int is_logits, int C, float (&p)[CM])
{
#pragma unroll
    for (int i = 0; i < CM; ++i) p[i] = i < C ? x[i] : 0.f;
    if (!is_logits) return;
    float m = p[0];
#pragma unroll
    for (int i = 1; i < CM; ++i) if (i < C) m = fmaxf(m, p[i]);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CM; ++i) if (i < C) { p[i] = expf(p[i] - m); s += p[i]; }
#pragma unroll
    for (int i = 0; i < CM; ++i) if (i < C) p[i] = p[i] / s;
}

// grid (chunks, nseg): a block's slots lie in one segment (blocked slots are image-major, as plain pixels are)
template <int CM>
__global__ __launch_bounds__(256) void lov_key_kernel(const float* __restrict__ x, int is_logits, const uint8_t* __restrict__ labels, const PixMap map,
                                                      long long slots_per_seg, long long L, int C, const uint8_t* __restrict__ mask,
                                                      unsigned* __restrict__ keys, unsigned* __restrict__ pays, unsigned* G, unsigned* V)
{
    __shared__ unsigned cg[CM], cv, msk[CM];
    if (threadIdx.x < CM) { cg[threadIdx.x] = 0; msk[threadIdx.x] = (int)threadIdx.x < C && (!mask || mask[threadIdx.x]); }
    if (threadIdx.x == 0) cv = 0;
    __syncthreads();
    const int s = blockIdx.y;
    const long long s0 = (long long)s * slots_per_seg;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < slots_per_seg; q += (long long)gridDim.x * blockDim.x) {
        const long long slot = s0 + q;
        const long long pix = slot_pixel(slot, map);
        if (pix < 0) continue;
        const long long i = pix - (long long)s * L;               // index inside the segment
        const int lab = labels[pix];
        const bool ign = lab >= C;
        float p[CM];
        lov_probs<CM>(x + slot * C, is_logits, C, p);
        if (!ign) { atomicAdd(&cv, 1u); if (msk[lab]) atomicAdd(&cg[lab], 1u); }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            if (!msk[c]) continue;
            const bool fg = c == lab;
            const float e = fg ? 1.f - p[c] : p[c];
            const size_t o = ((size_t)s * C + c) * (size_t)L + (size_t)i;
            keys[o] = ign ? LOV_IGNORE_KEY : 0x3F800000u - __float_as_uint(e);
            pays[o] = (unsigned)i | (fg ? 0x80000000u : 0u);
        }
    }
    __syncthreads();
    if (threadIdx.x < CM && msk[threadIdx.x] && cg[threadIdx.x]) atomicAdd(&G[s * C + threadIdx.x], cg[threadIdx.x]);
    if (threadIdx.x == 0 && cv) atomicAdd(&V[s], cv);
}

// one block: w[s][c] = 1 / (|S| |C_s|) for the participating classes of each segment, 0 elsewhere (double: the gradient's scale)
__global__ void lov_prep_kernel(const unsigned* G, int nseg, int C, const uint8_t* mask, int classes_all, double* w, int* ncls)
{
    for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
        int n = 0;
        for (int c = 0; c < C; ++c) n += (!mask || mask[c]) && (classes_all || G[s * C + c] > 0);
        ncls[s] = n;
        for (int c = 0; c < C; ++c) {
            const bool on = (!mask || mask[c]) && (classes_all || G[s * C + c] > 0);
            w[s * C + c] = on ? 1.0 / ((double)nseg * (double)n) : 0.0;
        }
    }
}

// grid (tiles, nsc): the tile's digit histogram -> hist[sc][tile][digit]
__global__ __launch_bounds__(256) void lov_hist_kernel(const unsigned* __restrict__ keys, long long L, int tiles, int shift, const double* w,
                                                       unsigned* __restrict__ hist)
{
    const int sc = blockIdx.y, tile = blockIdx.x;
    if (w[sc] == 0.0) return;
    __shared__ unsigned h[LOV_BINS];
    for (int i = threadIdx.x; i < LOV_BINS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const long long t0 = (long long)tile * LOV_TILE, t1 = t0 + LOV_TILE < L ? t0 + LOV_TILE : L;
    const unsigned* k = keys + (size_t)sc * L;
    for (long long j = t0 + threadIdx.x; j < t1; j += blockDim.x) atomicAdd(&h[(k[j] >> shift) & (LOV_BINS - 1)], 1u);
    __syncthreads();
    unsigned* o = hist + ((size_t)sc * tiles + tile) * LOV_BINS;
    for (int i = threadIdx.x; i < LOV_BINS; i += blockDim.x) o[i] = h[i];
}

// grid nsc, 1024 threads (thread = digit): exclusive scan of hist[sc] in (digit, tile) order, in place
__global__ __launch_bounds__(1024) void lov_scan_kernel(unsigned* hist, int tiles, const double* w)
{
    const int sc = blockIdx.x, d = threadIdx.x;
    if (w[sc] == 0.0) return;
    __shared__ unsigned sh[LOV_BINS];
    unsigned* h = hist + (size_t)sc * tiles * LOV_BINS;
    unsigned tot = 0;
    for (int t = 0; t < tiles; ++t) tot += h[(size_t)t * LOV_BINS + d];
    sh[d] = tot;
    __syncthreads();
    for (int off = 1; off < LOV_BINS; off <<= 1) {                  // inclusive Hillis-Steele scan of the digit totals
        const unsigned v = d >= off ? sh[d - off] : 0u;
        __syncthreads();
        sh[d] += v;
        __syncthreads();
    }
    unsigned run = sh[d] - tot;                                      // exclusive
    for (int t = 0; t < tiles; ++t) { const size_t o = (size_t)t * LOV_BINS + d; const unsigned c = h[o]; h[o] = run; run += c; }
}

// grid (tiles, nsc): stable scatter of one tile.  Rounds of 256 consecutive keys; a key's place = the tile's offset for its digit + the
// keys of that digit in earlier rounds + those in earlier waves of this round + its rank among its wave peers (equal digit, lower lane).
__global__ __launch_bounds__(256) void lov_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ pin, unsigned* __restrict__ kout,
                                                          unsigned* __restrict__ pout, long long L, int tiles, int shift, const unsigned* __restrict__ hist,
                                                          const double* w)
{
    const int sc = blockIdx.y, tile = blockIdx.x;
    if (w[sc] == 0.0) return;
    __shared__ unsigned run[LOV_BINS];
    __shared__ unsigned wcnt[4][LOV_BINS];
    const unsigned* h = hist + ((size_t)sc * tiles + tile) * LOV_BINS;
    for (int i = threadIdx.x; i < LOV_BINS; i += blockDim.x) { run[i] = h[i]; wcnt[0][i] = wcnt[1][i] = wcnt[2][i] = wcnt[3][i] = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const size_t base = (size_t)sc * L;
    const long long t0 = (long long)tile * LOV_TILE;
    for (int r = 0; r < LOV_IPT; ++r) {
        const long long j = t0 + (long long)r * 256 + threadIdx.x;
        if (t0 + (long long)r * 256 >= L) break;                     // block-uniform
        const bool valid = j < L;
        const unsigned key = valid ? kin[base + j] : 0u, pay = valid ? pin[base + j] : 0u;
        const unsigned d = (key >> shift) & (LOV_BINS - 1);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < LOV_BITS; ++b) {
            const unsigned long long bb = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? bb : ~bb;
        }
        const unsigned rank = (unsigned)__popcll(peers & lt), cnt = (unsigned)__popcll(peers);
        if (valid && rank == 0) wcnt[wave][d] = cnt;
        __syncthreads();
        if (valid) {
            unsigned pos = run[d] + rank;
            for (int v = 0; v < wave; ++v) pos += wcnt[v][d];
            kout[base + pos] = key; pout[base + pos] = pay;
        }
        __syncthreads();
        if (valid && rank == 0) { wcnt[wave][d] = 0; atomicAdd(&run[d], cnt); }    // (integer: the order of the adds does not matter)
    }
}

// grid (tiles, nsc): foreground pixels per sorted tile
__global__ __launch_bounds__(256) void lov_fgcount_kernel(const unsigned* __restrict__ pays, long long L, int tiles, const double* w, unsigned* tcnt)
{
    const int sc = blockIdx.y, tile = blockIdx.x;
    if (w[sc] == 0.0) return;
    __shared__ unsigned sh[4];
    const long long t0 = (long long)tile * LOV_TILE, t1 = t0 + LOV_TILE < L ? t0 + LOV_TILE : L;
    unsigned n = 0;
    for (long long j = t0 + threadIdx.x; j < t1; j += blockDim.x) n += pays[(size_t)sc * L + j] >> 31;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) tcnt[(size_t)sc * tiles + tile] = sh[0] + sh[1] + sh[2] + sh[3];
}

// grid (tiles, nsc): f_r by the two-level scan, g_r from the closed form (double, rounded to float once), the tile's sum of e g and the
// gradient plane dprob[c][s L + i] = g_r sgn(prob - fg) w[s][c] (scattered 4-byte stores)
__global__ __launch_bounds__(256) void lov_grad_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ pays, long long L, int tiles, int C,
                                                       long long P, const double* w, const unsigned* G, const unsigned* V, const unsigned* tcnt,
                                                       float* __restrict__ plane, double* part)
{
    const int sc = blockIdx.y, tile = blockIdx.x;
    const double ws = w[sc];
    if (ws == 0.0) return;
    __shared__ double dsh[4];
    __shared__ unsigned wt[4], fb[4];
    const int s = sc / C, c = sc % C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned f0 = 0;
    for (int t = threadIdx.x; t < tile; t += blockDim.x) f0 += tcnt[(size_t)sc * tiles + t];
    for (int o = 32; o > 0; o >>= 1) f0 += __shfl_down(f0, o, 64);
    if (lane == 0) fb[wave] = f0;
    __syncthreads();
    long long run = (long long)fb[0] + fb[1] + fb[2] + fb[3];     // foreground pixels in the earlier tiles
    const long long Gs = G[sc], Vs = V[s];
    const unsigned long long le = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull);
    const size_t base = (size_t)sc * L;
    float* pl = plane + (size_t)c * P + (size_t)s * L;
    double acc = 0;
    const long long t0 = (long long)tile * LOV_TILE;
    for (int r = 0; r < LOV_IPT; ++r) {
        const long long j0 = t0 + (long long)r * 256;
        if (j0 >= Vs) break;                                         // block-uniform: the ignored pixels sort last and are skipped
        const long long j = j0 + threadIdx.x;
        const bool valid = j < Vs;
        const unsigned key = valid ? keys[base + j] : 0u, pay = valid ? pays[base + j] : 0u;
        const bool fg = valid && (pay >> 31);
        const unsigned long long bal = __ballot(fg);
        if (lane == 0) wt[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        long long f = run + __popcll(bal & le);
        for (int v = 0; v < wave; ++v) f += wt[v];
        const long long tot = (long long)wt[0] + wt[1] + wt[2] + wt[3];
        __syncthreads();
        run += tot;
        if (!valid) continue;
        const long long rk = j + 1;                                  // 1-based rank
        double g;
        if (Gs == 0) g = rk == 1 ? 1.0 : 0.0;
        else if (fg) g = 1.0 / (double)(Gs + rk - f);
        else g = (double)(Gs - f) / ((double)(Gs + rk - 1 - f) * (double)(Gs + rk - f));
        const float gf = (float)g;
        const float e = __uint_as_float(0x3F800000u - key);
        acc += (double)e * (double)gf;
        const float q = e > 0.f ? (float)((double)gf * ws) : 0.f;    // sgn(prob - fg): -1 foreground, +1 background, 0 when e == 0
        pl[pay & 0x7FFFFFFFu] = fg ? -q : q;
    }
    const double t = lov_block_sum(acc, dsh);
    if (threadIdx.x == 0) part[(size_t)sc * tiles + tile] = t;
}

// one block: l_{s,c} = sum of the tile partials in order; the segment's mean over C_s; L_lov = the mean over the segments.  Writes
// lov_out[0], class_loss[s C + c] (0 for a class outside C_s; may be null) and, for the model, the total loss and the terms.
__global__ __launch_bounds__(256) void lov_finalize_kernel(const double* part, int nseg, int C, int tiles, const double* w, const int* ncls,
                                                           float* lov_out, float* class_loss, float* terms, float lce, float llov, float* loss_out)
{
    __shared__ double sh[4];
    __shared__ double segsum;
    double total = 0;
    for (int s = 0; s < nseg; ++s) {
        if (threadIdx.x == 0) segsum = 0;
        for (int c = 0; c < C; ++c) {
            const int sc = s * C + c;
            if (w[sc] == 0.0) { if (class_loss && threadIdx.x == 0) class_loss[sc] = 0.f; continue; }
            double v = 0;
            for (int t = threadIdx.x; t < tiles; t += blockDim.x) v += part[(size_t)sc * tiles + t];
            const double l = lov_block_sum(v, sh);
            if (threadIdx.x == 0) { segsum += l; if (class_loss) class_loss[sc] = (float)l; }
        }
        if (threadIdx.x == 0 && ncls[s] > 0) total += segsum / (double)ncls[s];
    }
    if (threadIdx.x == 0) {
        const float lov = (float)(total / (double)nseg);
        lov_out[0] = lov;
        if (terms) { terms[1] = lov; loss_out[0] = (lce * terms[0] + llov * lov) + terms[2]; }
    }
}

// the loss of a configuration without the Lovász term (lambda_lov == 0, lambda_ce != 1): lambda_ce ce + l2
__global__ void lov_total_kernel(float* terms, float lce, float* loss_out)
{
    if (threadIdx.x == 0) { terms[1] = 0.f; loss_out[0] = lce * terms[0] + terms[2]; }
}

// grid-stride over slots (fixed grid): q = the pixel's row of the gradient plane (0 outside C_s), then
//   logits: out += lambda prob (q - <q, prob>), per-block column sums of that contribution -> colpart[block][c]
//   probabilities: out = q
template <int CM>
__global__ __launch_bounds__(256) void lov_bwd_kernel(const float* __restrict__ x, int is_logits, const uint8_t* __restrict__ labels, const PixMap map,
                                                      long long nslot, long long L, long long P, int C, const double* __restrict__ w,
                                                      const float* __restrict__ plane, float lambda, int accumulate, float* __restrict__ out,
                                                      float* __restrict__ colpart)
{
    float cs[CM];
#pragma unroll
    for (int i = 0; i < CM; ++i) cs[i] = 0.f;
    for (long long slot = blockIdx.x * (long long)blockDim.x + threadIdx.x; slot < nslot; slot += (long long)gridDim.x * blockDim.x) {
        const long long pix = slot_pixel(slot, map);
        if (pix < 0) continue;                                       // (a slot outside the image keeps its zero gradient)
        const int lab = labels[pix];
        float* o = out + slot * C;
        if (lab >= C) { if (!accumulate) for (int i = 0; i < C; ++i) o[i] = 0.f; continue; }
        const int s = (int)(pix / L);
        float q[CM];
#pragma unroll
        for (int i = 0; i < CM; ++i) q[i] = (i < C && w[(size_t)s * C + i] != 0.0) ? plane[(size_t)i * P + pix] : 0.f;
        if (!is_logits) {
#pragma unroll
            for (int i = 0; i < CM; ++i) if (i < C) o[i] = accumulate ? o[i] + lambda * q[i] : lambda * q[i];
            continue;
        }
        float p[CM];
        lov_probs<CM>(x + slot * C, 1, C, p);
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < CM; ++i) if (i < C) dot += q[i] * p[i];
#pragma unroll
        for (int i = 0; i < CM; ++i) if (i < C) {
            const float t = lambda * (p[i] * (q[i] - dot));
            o[i] = accumulate ? o[i] + t : t;
            cs[i] += t;
        }
    }
    if (!colpart) return;
    __shared__ float sh[4][CM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < CM; ++i) {
        float v = cs[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sh[wave][i] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) colpart[(size_t)blockIdx.x * C + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// grid C: one block per class, the partials strided over the threads and tree-reduced in a fixed order
__global__ __launch_bounds__(256) void lov_colsum_kernel(const float* colpart, int nblocks, int C, float* colsum)
{
    __shared__ float sh[4];
    const int c = blockIdx.x;
    float v = 0.f;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) v += colpart[(size_t)b * C + c];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) colsum[c] += ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

constexpr int LOV_BWD_BLOCKS = 2048;

}  // namespace

// ---- host side --------------------------------------------------------------------------------------------------------------------
LovaszLayout lovasz_layout(long long npix, int nseg, int C)
{
    LovaszLayout y{};
    y.nseg = nseg; y.C = C; y.L = npix / nseg; y.nsc = (long long)nseg * C;
    y.tiles = (int)((y.L + LOV_TILE - 1) / LOV_TILE);
    const size_t n = (size_t)y.nsc * (size_t)y.L;
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += (b + 255) / 256 * 256; return at; };
    y.o_keys[0] = take(n * 4); y.o_pays[0] = take(n * 4); y.o_keys[1] = take(n * 4); y.o_pays[1] = take(n * 4);
    y.o_hist = take((size_t)y.nsc * y.tiles * LOV_BINS * 4);
    y.o_tcnt = take((size_t)y.nsc * y.tiles * 4);
    y.o_part = take((size_t)y.nsc * y.tiles * 8);
    y.o_G = take((size_t)y.nsc * 4); y.o_V = take((size_t)nseg * 4);
    y.o_w = take((size_t)y.nsc * 8); y.o_ncls = take((size_t)nseg * 4);
    y.o_colpart = take((size_t)LOV_BWD_BLOCKS * 64 * 4);
    y.o_lov = take(64);
    y.bytes = o;
    return y;
}

double lovasz_bytes(long long npix, int C, int nmask)
{
    const double n = (double)npix * nmask;
    // logits + labels, keys + payloads written, three passes (histogram read, scatter read + write), the foreground count, the scan
    // pass (read keys + payloads, write the plane), the backward (logits, plane, labels, dlogits read + write)
    return (double)npix * (C * 4.0 + 1) + 8 * n + 3 * (4 * n + 16 * n) + 4 * n + 12 * n + (double)npix * (C * 4.0 * 4 + 1);
}

template <int CM>
static void lov_launch_keys_bwd(bool bwd, const float* x, int is_logits, const uint8_t* labels, const PixMap& pm, long long nslot, const LovaszLayout& y,
                                long long P, const uint8_t* mask, char* ws, float lambda, int accumulate, float* out, float* colpart, hipStream_t s)
{
    if (!bwd) {
        const long long sps = nslot / y.nseg;
        long long bx = (sps + 255) / 256; if (bx > 1024) bx = 1024; if (bx < 1) bx = 1;
        hipLaunchKernelGGL((lov_key_kernel<CM>), dim3((unsigned)bx, y.nseg), dim3(256), 0, s, x, is_logits, labels, pm, sps, y.L, y.C, mask,
                           (unsigned*)(ws + y.o_keys[0]), (unsigned*)(ws + y.o_pays[0]), (unsigned*)(ws + y.o_G), (unsigned*)(ws + y.o_V));
    } else {
        hipLaunchKernelGGL((lov_bwd_kernel<CM>), dim3(LOV_BWD_BLOCKS), dim3(256), 0, s, x, is_logits, labels, pm, nslot, y.L, P, y.C,
                           (const double*)(ws + y.o_w), (const float*)(ws + y.o_keys[0]), lambda, accumulate, out, colpart);
    }
}

static void lov_dispatch(bool bwd, const float* x, int is_logits, const uint8_t* labels, const PixMap& pm, long long nslot, const LovaszLayout& y,
                         long long P, const uint8_t* mask, char* ws, float lambda, int accumulate, float* out, float* colpart, hipStream_t s)
{
    const int C = y.C;
    if (C <= 4)       lov_launch_keys_bwd<4>(bwd, x, is_logits, labels, pm, nslot, y, P, mask, ws, lambda, accumulate, out, colpart, s);
    else if (C <= 12) lov_launch_keys_bwd<12>(bwd, x, is_logits, labels, pm, nslot, y, P, mask, ws, lambda, accumulate, out, colpart, s);
    else if (C <= 20) lov_launch_keys_bwd<20>(bwd, x, is_logits, labels, pm, nslot, y, P, mask, ws, lambda, accumulate, out, colpart, s);
    else if (C <= 32) lov_launch_keys_bwd<32>(bwd, x, is_logits, labels, pm, nslot, y, P, mask, ws, lambda, accumulate, out, colpart, s);
    else              lov_launch_keys_bwd<64>(bwd, x, is_logits, labels, pm, nslot, y, P, mask, ws, lambda, accumulate, out, colpart, s);
}

void launch_lovasz_loss(const float* x, int is_logits, const uint8_t* labels, const PixMap* map, int N, long long npix, const LovaszLayout& y,
                        int classes_all, const uint8_t* mask_dev, char* ws, float* class_loss, float* terms, float lce, float llov, float* loss_out,
                        hipStream_t s)
{
    const PixMap pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    const long long nslot = pixmap_slots(pm, npix, N);
    unsigned* G = (unsigned*)(ws + y.o_G);
    hipMemsetAsync(ws + y.o_G, 0, (size_t)y.nsc * 4, s);
    hipMemsetAsync(ws + y.o_V, 0, (size_t)y.nseg * 4, s);
    lov_dispatch(false, x, is_logits, labels, pm, nslot, y, npix, mask_dev, ws, 0.f, 0, nullptr, nullptr, s);
    double* w = (double*)(ws + y.o_w);
    hipLaunchKernelGGL(lov_prep_kernel, dim3(1), dim3(256), 0, s, (const unsigned*)G, y.nseg, y.C, mask_dev, classes_all, w, (int*)(ws + y.o_ncls));
    const dim3 grid((unsigned)y.tiles, (unsigned)y.nsc);
    unsigned* hist = (unsigned*)(ws + y.o_hist);
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass * LOV_BITS, a = pass & 1, b = a ^ 1;
        const unsigned* kin = (const unsigned*)(ws + y.o_keys[a]); const unsigned* pin = (const unsigned*)(ws + y.o_pays[a]);
        hipLaunchKernelGGL(lov_hist_kernel, grid, dim3(256), 0, s, kin, y.L, y.tiles, shift, (const double*)w, hist);
        hipLaunchKernelGGL(lov_scan_kernel, dim3((unsigned)y.nsc), dim3(1024), 0, s, hist, y.tiles, (const double*)w);
        hipLaunchKernelGGL(lov_scatter_kernel, grid, dim3(256), 0, s, kin, pin, (unsigned*)(ws + y.o_keys[b]), (unsigned*)(ws + y.o_pays[b]), y.L, y.tiles,
                           shift, (const unsigned*)hist, (const double*)w);
    }
    // sorted in buffer 1; buffer 0's keys become the gradient plane
    const unsigned* ks = (const unsigned*)(ws + y.o_keys[1]); const unsigned* ps = (const unsigned*)(ws + y.o_pays[1]);
    unsigned* tcnt = (unsigned*)(ws + y.o_tcnt);
    hipLaunchKernelGGL(lov_fgcount_kernel, grid, dim3(256), 0, s, ps, y.L, y.tiles, (const double*)w, tcnt);
    hipLaunchKernelGGL(lov_grad_kernel, grid, dim3(256), 0, s, ks, ps, y.L, y.tiles, y.C, npix, (const double*)w, (const unsigned*)G,
                       (const unsigned*)(ws + y.o_V), (const unsigned*)tcnt, (float*)(ws + y.o_keys[0]), (double*)(ws + y.o_part));
    hipLaunchKernelGGL(lov_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)(ws + y.o_part), y.nseg, y.C, y.tiles, (const double*)w,
                       (const int*)(ws + y.o_ncls), (float*)(ws + y.o_lov), class_loss, terms, lce, llov, loss_out);
}

void launch_lovasz_backward(const float* x, int is_logits, const uint8_t* labels, const PixMap* map, int N, long long npix, const LovaszLayout& y,
                            char* ws, float lambda, int accumulate, float* out, float* colsum, hipStream_t s)
{
    const PixMap pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    const long long nslot = pixmap_slots(pm, npix, N);
    float* colpart = colsum ? (float*)(ws + y.o_colpart) : nullptr;
    lov_dispatch(true, x, is_logits, labels, pm, nslot, y, npix, nullptr, ws, lambda, accumulate, out, colpart, s);
    if (colsum) hipLaunchKernelGGL(lov_colsum_kernel, dim3(y.C), dim3(256), 0, s, (const float*)colpart, LOV_BWD_BLOCKS, y.C, colsum);
}

void launch_lovasz_total(float* terms, float lce, float* loss_out, hipStream_t s)
{
    hipLaunchKernelGGL(lov_total_kernel, dim3(1), dim3(64), 0, s, terms, lce, loss_out);
}

}  // namespace fcn8s
