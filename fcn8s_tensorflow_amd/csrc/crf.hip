// Mean-field refinement of a softmax by a locally connected CRF (fcn8s_op_crf_meanfield / fcn8s_predict_crf; the definition is in
// include/fcn8s_hip.h and, in float64, in fcn8s_tensorflow_amd/crf.py).
//   crf_meanfield_kernel : one Jacobi update Q^{t-1} -> Q^t.  Pixels with equal (y mod d, x mod d) form d*d independent sub-images and a window of
//                          dilation d on the image is an undilated one on each of them, so a block owns a 32 x TY tile of ONE sub-image and its halo
//                          is r pixels for every d.  The tile plus halo of Q^{t-1} is staged in LDS class-planar ([C/4][pixel] float4: the lanes of
//                          a ds_read_b128 then read consecutive 16-byte slots), the image as one packed dword per pixel (r | g << 8 | b << 16 |
//                          inside-the-image << 24).  Pixels outside the image are staged as Q = 0, flag 0: they add nothing to a message and
//                          nothing to the position-only divisors.  One thread owns one pixel: it walks the (2r+1)^2 taps in row-major order,
//                          four at a time (the centre and the entries that fill the last four carry weight 0), with the C accumulators of both
//                          messages in registers (v_pk_fma_f32), takes the position-only factors from a per-launch table in the kernel
//                          arguments (uniform index: scalar loads, no expf), spends one v_exp_f32 per tap on the colour factor, and ends
//                          with the unary, the softmax and 16-byte stores.  The image is staged with byte loads (3 of the 243 bytes a pixel
//                          moves).  No atomics, one summation order: two runs give the same bits.
//   crf_argmax_kernel    : iterations = 0 with an argmax output (the argmax of P itself).
// C = 20 and C = 4 keep every class in registers; any other multiple of 4 sweeps the taps once per group of 4 classes and parks the pre-softmax
// values in the output row of its own pixel between the sweeps.
#include "fcn8s_internal.h"
#include <cfloat>
#include <cmath>

namespace fcn8s {

#define CRF_TX 32           // a wave covers two rows of 32 pixels: every lane group of a ds_read_b128 reads consecutive 16-byte slots of one row
#define CRF_MAX_TAPS 225    // (2 * 7 + 1)^2

struct CrfGeom {
    int N, H, W, C, r, d;
    float neg_inv_2beta2_log2e;          // -log2(e) / (2 theta_beta^2): exp(-c2 / (2 theta_beta^2)) is one v_exp_f32 of c2 times this
    float w_app, w_smooth;
};

// two classes per register pair: the messages are summed with v_pk_fma_f32 (measured: the same sums as v_fma_f32 take 19-24 % longer here)
typedef float crf_f2 __attribute__((ext_vector_type(2)));

#define CRF_CHUNK 4      // taps summed per trip of the loop: their packed pixels and weights are independent work in flight together
#define CRF_TAB ((CRF_MAX_TAPS + CRF_CHUNK - 1) / CRF_CHUNK * CRF_CHUNK)
// per launch, in the kernel arguments (the tap index is uniform: scalar loads): (a_ij, g_ij) = (exp(-s2 / (2 theta_alpha^2)), exp(-s2 / (2 theta_gamma^2)))
// of the (2r+1)^2 taps in row-major order, s2 in pixels of the image; (0, 0) for the centre and for the entries that fill the last chunk
struct CrfTable { float2 ag[CRF_TAB]; };

// both messages' sums over the window of the pixel whose window starts at LDS pixel `base` (= ly * tw + lx), for the NC classes that start at plane `q`
// (NC / 4 planes of tp float4 each); sa / sg: the position-only divisors.  One flat loop over the taps, CRF_CHUNK at a time; a filling entry reads a
// clamped, valid LDS pixel with weight 0.
template <int NC>
static __device__ __forceinline__ void crf_sweep(const float4* __restrict__ q, const uint32_t* __restrict__ pix, const CrfTable& tab, int n, int tw,
                                                 int tp, int base, uint32_t cp, float neg_inv_2beta2_log2e, crf_f2 (&A)[NC / 2], crf_f2 (&G)[NC / 2],
                                                 float& sa, float& sg)
{
    const float cr = (float)(cp & 255u), cg = (float)((cp >> 8) & 255u), cb = (float)((cp >> 16) & 255u);
#pragma unroll
    for (int i = 0; i < NC / 2; ++i) { A[i] = crf_f2{0.f, 0.f}; G[i] = crf_f2{0.f, 0.f}; }
    crf_f2 sd = crf_f2{0.f, 0.f};
    int tx = 0, off = 0;                                                   // (uniform) column of the tap, its LDS offset from `base`
    for (int t = 0; t < n * n; t += CRF_CHUNK) {
        int p[CRF_CHUNK]; uint32_t np[CRF_CHUNK]; float wk[CRF_CHUNK], wg[CRF_CHUNK];
#pragma unroll
        for (int j = 0; j < CRF_CHUNK; ++j) {
            p[j] = min(base + off, tp - 1); np[j] = pix[p[j]];
            ++tx; ++off;
            if (tx == n) { tx = 0; off += tw - n; }
        }
#pragma unroll
        for (int j = 0; j < CRF_CHUNK; ++j) {
            const float2 e = tab.ag[t + j];
            const float dr = (float)(np[j] & 255u) - cr, dg = (float)((np[j] >> 8) & 255u) - cg, db = (float)((np[j] >> 16) & 255u) - cb;
            const float c2 = dr * dr + dg * dg + db * db;                  // integers below 2^24: exact, fused or not
            const bool in = (np[j] >> 24) != 0u;
            const crf_f2 wp = crf_f2{in ? e.x : 0.f, in ? e.y : 0.f};      // (position-only: a_ij, g_ij)
            wk[j] = wp.x * __builtin_amdgcn_exp2f(c2 * neg_inv_2beta2_log2e);
            wg[j] = wp.y;
            sd += wp;
        }
#pragma unroll
        for (int j = 0; j < CRF_CHUNK; ++j) {
            const crf_f2 k2 = crf_f2{wk[j], wk[j]}, g2 = crf_f2{wg[j], wg[j]};
#pragma unroll
            for (int i = 0; i < NC / 4; ++i) {
                const float4 v = q[i * tp + p[j]];
                const crf_f2 lo = crf_f2{v.x, v.y}, hi = crf_f2{v.z, v.w};
                A[2 * i] = __builtin_elementwise_fma(k2, lo, A[2 * i]); A[2 * i + 1] = __builtin_elementwise_fma(k2, hi, A[2 * i + 1]);
                G[2 * i] = __builtin_elementwise_fma(g2, lo, G[2 * i]); G[2 * i + 1] = __builtin_elementwise_fma(g2, hi, G[2 * i + 1]);
            }
        }
    }
    sa = sd.x; sg = sd.y;
}

// CT > 0: C == CT, all classes in registers.  CT == 0: any C % 4 == 0, four classes per sweep.
template <int CT>
__global__ __launch_bounds__(512) void crf_meanfield_kernel(const float* __restrict__ qin, const float* __restrict__ prob, const unsigned char* __restrict__ img,
                                                            const CrfGeom g, const CrfTable tab, float* qout, long long* __restrict__ am)
{
    extern __shared__ float4 crf_lds[];
    const int r = g.r, d = g.d, H = g.H, W = g.W;
    const int C = CT > 0 ? CT : g.C, C4 = C / 4;
    const int TY = blockDim.x / CRF_TX, tw = CRF_TX + 2 * r, th = TY + 2 * r, tp = tw * th;
    uint32_t* pix = reinterpret_cast<uint32_t*>(crf_lds + C4 * tp);        // tp dwords
    // block -> image n, sub-image (y0, x0) of Hs x Ws pixels, tile origin (ty0, tx0) in the sub-image's coordinates
    int z = blockIdx.z;
    const int n = z / (d * d); z -= n * d * d;
    const int y0 = z / d, x0 = z - y0 * d;
    const int Hs = y0 < H ? (H - y0 + d - 1) / d : 0, Ws = x0 < W ? (W - x0 + d - 1) / d : 0;
    const int ty0 = blockIdx.y * TY, tx0 = blockIdx.x * CRF_TX;
    if (ty0 >= Hs || tx0 >= Ws) return;                                    // (the whole block: the grid is sized for sub-image (0, 0), the largest)
    const int tid = threadIdx.x, lane = tid & 63, nwaves = blockDim.x >> 6;
    // stage: a wave per tile row, lanes over (pixel, class group) with the class group fastest (16-byte global loads, contiguous per pixel)
    for (int py = tid >> 6; py < th; py += nwaves) {
        const int sy = ty0 + py - r;
        const bool rin = sy >= 0 && sy < Hs;
        const long long row = ((long long)n * H + (y0 + (long long)sy * d)) * W;
        for (int j = lane; j < tw * C4; j += 64) {
            const int px = j / C4, c4 = j - px * C4, sx = tx0 + px - r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rin && sx >= 0 && sx < Ws) v = reinterpret_cast<const float4*>(qin + (row + x0 + (long long)sx * d) * C)[c4];
            crf_lds[c4 * tp + py * tw + px] = v;
        }
        for (int px = lane; px < tw; px += 64) {
            const int sx = tx0 + px - r;
            uint32_t v = 0u;
            if (rin && sx >= 0 && sx < Ws) {
                const unsigned char* q = img + (row + x0 + (long long)sx * d) * 3;
                v = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | (1u << 24);
            }
            pix[py * tw + px] = v;
        }
    }
    __syncthreads();
    const int ly = tid / CRF_TX, lx = tid - ly * CRF_TX;
    const int sy = ty0 + ly, sx = tx0 + lx;
    if (sy >= Hs || sx >= Ws) return;
    const long long pi = ((long long)n * H + (y0 + sy * d)) * W + (x0 + sx * d);
    const float4* pp = reinterpret_cast<const float4*>(prob + pi * C);
    float4* qo = reinterpret_cast<float4*>(qout + pi * C);
    float sa, sg;
    const int base = ly * tw + lx;
    const uint32_t cp = pix[base + r * tw + r];
    if constexpr (CT > 0) {
        constexpr int NC = CT > 0 ? CT : 4;
        crf_f2 A[NC / 2], G[NC / 2];
        crf_sweep<NC>(crf_lds, pix, tab, 2 * r + 1, tw, tp, base, cp, g.neg_inv_2beta2_log2e, A, G, sa, sg);
        const float ia = sa > 0.f ? g.w_app / sa : 0.f, ig = sg > 0.f ? g.w_smooth / sg : 0.f;
        float x[NC];
#pragma unroll
        for (int i = 0; i < NC / 4; ++i) {
            const float4 u = pp[i];
            x[4*i]   = logf(fmaxf(u.x, FLT_MIN)) + (ia * A[2*i].x   + ig * G[2*i].x);
            x[4*i+1] = logf(fmaxf(u.y, FLT_MIN)) + (ia * A[2*i].y   + ig * G[2*i].y);
            x[4*i+2] = logf(fmaxf(u.z, FLT_MIN)) + (ia * A[2*i+1].x + ig * G[2*i+1].x);
            x[4*i+3] = logf(fmaxf(u.w, FLT_MIN)) + (ia * A[2*i+1].y + ig * G[2*i+1].y);
        }
        float mx = x[0];
#pragma unroll
        for (int i = 1; i < NC; ++i) mx = fmaxf(mx, x[i]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) { x[i] = expf(x[i] - mx); s += x[i]; }
        const float is = 1.f / s;
        int best = 0; float bv = -1.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) { x[i] = x[i] * is; if (x[i] > bv) { bv = x[i]; best = i; } }
#pragma unroll
        for (int i = 0; i < NC / 4; ++i) qo[i] = make_float4(x[4*i], x[4*i+1], x[4*i+2], x[4*i+3]);
        if (am) am[pi] = best;
    } else {
        float mx = -FLT_MAX;
        for (int c4 = 0; c4 < C4; ++c4) {
            crf_f2 A[2], G[2];
            crf_sweep<4>(crf_lds + c4 * tp, pix, tab, 2 * r + 1, tw, tp, base, cp, g.neg_inv_2beta2_log2e, A, G, sa, sg);
            const float ia = sa > 0.f ? g.w_app / sa : 0.f, ig = sg > 0.f ? g.w_smooth / sg : 0.f;
            const float4 u = pp[c4];
            float4 x;
            x.x = logf(fmaxf(u.x, FLT_MIN)) + (ia * A[0].x + ig * G[0].x);
            x.y = logf(fmaxf(u.y, FLT_MIN)) + (ia * A[0].y + ig * G[0].y);
            x.z = logf(fmaxf(u.z, FLT_MIN)) + (ia * A[1].x + ig * G[1].x);
            x.w = logf(fmaxf(u.w, FLT_MIN)) + (ia * A[1].y + ig * G[1].y);
            mx = fmaxf(fmaxf(mx, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
            qo[c4] = x;                                                    // parked in this pixel's own output row (read back by this thread only)
        }
        float s = 0.f;
        for (int c4 = 0; c4 < C4; ++c4) {
            float4 x = qo[c4];
            x.x = expf(x.x - mx); x.y = expf(x.y - mx); x.z = expf(x.z - mx); x.w = expf(x.w - mx);
            s += x.x; s += x.y; s += x.z; s += x.w;
            qo[c4] = x;
        }
        const float is = 1.f / s;
        int best = 0; float bv = -1.f;
        for (int c4 = 0; c4 < C4; ++c4) {
            float4 x = qo[c4];
            x.x = x.x * is; x.y = x.y * is; x.z = x.z * is; x.w = x.w * is;
            if (x.x > bv) { bv = x.x; best = 4 * c4; }
            if (x.y > bv) { bv = x.y; best = 4 * c4 + 1; }
            if (x.z > bv) { bv = x.z; best = 4 * c4 + 2; }
            if (x.w > bv) { bv = x.w; best = 4 * c4 + 3; }
            qo[c4] = x;
        }
        if (am) am[pi] = best;
    }
}

__global__ __launch_bounds__(256) void crf_argmax_kernel(const float* __restrict__ p, long long npix, int C, long long* __restrict__ am)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const float* q = p + i * C;
        int best = 0; float bv = q[0];
        for (int c = 1; c < C; ++c) if (q[c] > bv) { bv = q[c]; best = c; }
        am[i] = best;
    }
}

void launch_crf_argmax(const float* p, long long npix, int C, long long* am, hipStream_t s)
{
    long long b = (npix + 255) / 256;
    hipLaunchKernelGGL(crf_argmax_kernel, dim3((unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b))), dim3(256), 0, s, p, npix, C, am);
}

// LDS of a 16 x ty tile with its halo: C floats of Q and one packed dword of the image per pixel, 
static size_t crf_lds_bytes(int C, int r, int ty)
{
    return (size_t)(CRF_TX + 2 * r) * (ty + 2 * r) * (4 * (size_t)C + 4);
}

// rows of the tile (threads = 32 * rows): of 2, 4, 8 and 16 the one that puts the most waves on a CU's 160 KB, the smaller on a tie (more blocks: one stages
// while another sums; measured at C = 20: radius 3 -> 16 rows, 0.243 ms per update of 2 Mpixel against 0.268 with 8; radius 5 -> 8 rows, 0.617 against 0.661
// with 16); 0: nothing fits
static int crf_tile_rows(int C, int r)
{
    int best = 0; size_t waves = 0;
    for (int ty = 2; ty <= 16; ty <<= 1) {
        const size_t b = crf_lds_bytes(C, r, ty), w = b <= FCN8S_LDS_BYTES_NEEDED ? FCN8S_LDS_BYTES_NEEDED / b * (size_t)(ty / 2) : 0;
        if (w > waves) { waves = w; best = ty; }
    }
    return best;
}
bool crf_shape_supported(int C, int r) { return C > 0 && C % 4 == 0 && crf_tile_rows(C, r) > 0; }

template <int CT>
static void crf_launch(const float* qin, const float* prob, const unsigned char* img, const CrfGeom& g, const CrfTable& tab, float* qout, long long* am,
                       int ty, size_t lds, hipStream_t s)
{
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&crf_meanfield_kernel<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "crf_meanfield: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return; }
    }
    const int ws = (g.W + g.d - 1) / g.d, hs = (g.H + g.d - 1) / g.d;
    const dim3 grid((ws + CRF_TX - 1) / CRF_TX, (hs + ty - 1) / ty, g.N * g.d * g.d);
    hipLaunchKernelGGL(crf_meanfield_kernel<CT>, grid, dim3(CRF_TX * ty), lds, s, qin, prob, img, g, tab, qout, am);
}

void launch_crf_meanfield(const float* qin, const float* prob, const unsigned char* img, int N, int H, int W, int C, int radius, int dilation,
                          float w_app, float w_smooth, float theta_alpha, float theta_beta, float theta_gamma, float* qout, long long* am, hipStream_t s)
{
    const int ty = crf_shape_supported(C, radius) ? crf_tile_rows(C, radius) : 0;
    if (!ty) { defer_error(FCN8S_ERR_SHAPE, "crf_meanfield: C = %d at radius %d does not fit the LDS tile (C must be a multiple of 4)", C, radius); return; }
    if ((long long)N * dilation * dilation > 65535 || (H + dilation - 1) / dilation / ty >= 65535) {
        defer_error(FCN8S_ERR_SHAPE, "crf_meanfield: N * dilation^2 and the tile rows must stay below 65535"); return;
    }
    CrfGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.r = radius; g.d = dilation;
    g.w_app = w_app; g.w_smooth = w_smooth;
    const float ia = 1.f / (2.f * theta_alpha * theta_alpha), ig = 1.f / (2.f * theta_gamma * theta_gamma);
    CrfTable tab;
    const int n = 2 * radius + 1;
    for (int t = 0; t < CRF_TAB; ++t) {
        const int y = t / n - radius, x = t % n - radius;
        const float s2 = (float)((y * y + x * x) * dilation * dilation);
        tab.ag[t] = t >= n * n || (y == 0 && x == 0) ? make_float2(0.f, 0.f) : make_float2(expf(-(s2 * ia)), expf(-(s2 * ig)));
    }
    g.neg_inv_2beta2_log2e = -1.44269504088896341f * (1.f / (2.f * theta_beta * theta_beta));
    const size_t lds = crf_lds_bytes(C, radius, ty);
    if (C == 20) crf_launch<20>(qin, prob, img, g, tab, qout, am, ty, lds, s);
    else if (C == 4) crf_launch<4>(qin, prob, img, g, tab, qout, am, ty, lds, s);
    else crf_launch<0>(qin, prob, img, g, tab, qout, am, ty, lds, s);
}

}  // namespace fcn8s
