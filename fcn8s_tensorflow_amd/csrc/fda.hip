// Fourier domain adaptation (fcn8s_op_fda_transfer; the definition is in fcn8s_hip.h; Yang & Soatto, CVPR 2020): the amplitudes of the (2 b + 1)^2
// lowest frequencies of every source image are replaced by those of its target image, the phases stay.  No FFT: only that window of coefficients
// changes, so the op is a partial DFT (two skinny GEMMs per image), a few thousand complex scalars, and a low-rank synthesis (two skinny GEMMs back)
// added onto the source.  A real image has F(-u, -v) = conj F(u, v), so only the columns v = 0 .. b are computed; the other half of the window
// enters the synthesis as a factor 2 on v >= 1.  With CP = 2 (b + 1) real columns (cos, sin per v) and B = 2 b + 1:
//
// Six kernels, split at kernel boundaries: no ticket, no fence, no float atomic, no block that waits for another, every loop bounded, every sum in
// a fixed order that depends on H, W and b only -- never on N, M or an image's place in the batch.
//   prep     the twiddle tables (cos, sin)(2 pi k / n) for n = W and n = H, each entry from sincospi in double of the reduced phase 2 k / n, rounded
//            to float; block 0 resolves pair[] (out of range: n mod M and the flag), and marks the targets that a source refers to.
//   rowdft   G[h][c][v] = sum_w x[h][w][c] e^{-2 pi i v w / W}: the real GEMM [rows x W] . [W x CP] on v_mfma_f32_32x32x2_f32, for the N sources and the
//            referenced targets alike (one instruction sequence: equal bytes give equal bits).  A block owns 32 rows of an image; per chunk of 64
//            pixels it stages the rows' bytes as whole 16-byte lines, a lane per line (the house pattern of strong_augment.hip), turns them into
//            floats [channel][k][row] in LDS (a row is the MFMA's M index, a channel one 32-row M tile); a block multiplies them into two column tiles of
//            32 (the third grid dimension walks the pairs of tiles), its four waves deal the MFMA steps of a chunk among themselves -- wave w the pixel
//            pairs w, w + 4, ... -- and their sums meet in LDS at the end, added in wave order.  The twiddle of (v, w) is read from the table at the phase
//            (v w) mod W, which a lane steps by 8 v per MFMA.
//   coldft   F[u][c][v] = sum_h e^{-2 pi i u h / H} G[h][c][v] in double: a block takes one u and up to 64 (c, v); the rows are dealt to 256 / 64 or
//            more slices whose sums meet in LDS and are added in slice order.
//   delta    D = phi (A_t - A_s) c_v / (H W) in double, stored as float; phi = F_s / A_s, 1 where A_s = 0; c_0 = 1, c_v = 2.  Equal spectra: exactly 0.
//   zsyn     S[h][c][2 v] = Re Z, S[h][c][2 v + 1] = -Im Z with Z[h][c][v] = sum_u e^{+2 pi i u h / H} D[u][c][v] (u ascending, fmaf chain); S lies
//            over the sources' G, which is dead by then.
//   synth    y[h][w][c] = x + sum_j S[h][c][j] T[j][w], T = (cos, sin)(2 pi v w / W): the real GEMM with K = CP on the same MFMA.  A block owns 32 rows
//            x 128 pixels: wave w the 32 pixels w, three accumulators (channels); S goes through LDS in chunks of 32 columns, [channel][j][row]; the
//            source bytes are staged as in rowdft, a lane ends up with whole pixels of 16 rows, and the bytes leave through an output strip as whole
//            16-byte lines, byte by byte at a row's ragged ends.  out_f32 is stored directly (32 lanes = 384 consecutive bytes).
#include "fcn8s_internal.h"

namespace fcn8s {

typedef float fda_f32x16 __attribute__((ext_vector_type(16)));

#define FDA_THREADS 256
#define FDA_RT 32                                    // rows per block (both GEMM kernels): the MFMA's M
#define FDA_KC 64                                    // rowdft: pixels per chunk
#define FDA_RS1 208                                  // rowdft: bytes per staged row: 15 + 3 * 64 in whole lines
#define FDA_TW 128                                   // synth: pixels per block
#define FDA_RS2 400                                  // synth: bytes per staged row and per row of the output strip: 15 + 3 * 128 in whole lines
#define FDA_JC 32                                    // synth: columns of S per chunk
#define FDA_QW 64                                    // coldft / zsyn: complex columns per block

struct FdaLayout { size_t pr, used, tww, twh, g, f, d, total; };
__host__ __device__ static inline size_t fda_up16(size_t x) { return (x + 15) & ~(size_t)15; }
// offsets from the first 16-byte boundary of work: the flag (16 bytes), pr int[256], used int[256], the two tables, G (S over its first N images), F, D
static inline FdaLayout fda_layout(int N, int M, int H, int W, int b)
{
    const size_t CP = 2 * ((size_t)b + 1), B = 2 * (size_t)b + 1, Q = 3 * ((size_t)b + 1);
    FdaLayout l;
    l.pr = 16;
    l.used = l.pr + 1024;
    l.tww = l.used + 1024;
    l.twh = l.tww + fda_up16((size_t)W * 8);
    l.g = l.twh + fda_up16((size_t)H * 8);
    l.f = l.g + fda_up16((size_t)(N + M) * H * 3 * CP * 4);
    l.d = l.f + (size_t)(N + M) * B * Q * 16;
    l.total = l.d + fda_up16((size_t)N * B * Q * 8);
    return l;
}
size_t fda_work_bytes(int N, int M, int H, int W, int b)
{
    if (N <= 0 || M <= 0 || H <= 0 || W <= 0 || b < 0) return 0;
    return 16 + fda_layout(N, M, H, W, b).total;
}

// grid: enough blocks of 256 for max(H, W)
__global__ __launch_bounds__(FDA_THREADS) void fda_prep_kernel(int N, int M, int H, int W, const int* __restrict__ pair, unsigned int* flag, int* pr, int* used,
                                                              float2* tww, float2* twh)
{
    const int t = threadIdx.x;
    const long long i = (long long)blockIdx.x * FDA_THREADS + t;
    if (i < W) { double s, c; sincospi(2.0 * (double)i / (double)W, &s, &c); tww[i] = make_float2((float)c, (float)s); }
    if (i < H) { double s, c; sincospi(2.0 * (double)i / (double)H, &s, &c); twh[i] = make_float2((float)c, (float)s); }
    if (blockIdx.x == 0) {
        __shared__ int us[256];
        us[t] = 0;
        __syncthreads();
        int bad = 0;
        if (t < N) {
            int p = pair ? pair[t] : t % M;
            if (p < 0 || p >= M) { bad = 1; p = t % M; }
            pr[t] = p;
            us[p] = 1;                                           // (several sources of one target store the same 1)
        }
        bad = __syncthreads_or(bad);
        used[t] = us[t];
        if (t == 0) *flag = bad ? 1u : 0u;
    }
}

// the 16-byte line of global memory at g; where it sticks out of the tensor [lo, hi), its bytes inside
__device__ __forceinline__ uint4 fda_fetch(uintptr_t lo, uintptr_t hi, uintptr_t g)
{
    if (g >= lo && g + 16 <= hi) return *reinterpret_cast<const uint4*>(g);
    unsigned int w[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < 16; ++j)
        if (g + j >= lo && g + j < hi) w[j >> 2] |= (unsigned int)*reinterpret_cast<const uint8_t*>(g + j) << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// stages `len` bytes of each of `rows` image rows (row r begins at row0 + r * pitch) into raw[r][RS] as whole lines, a lane per line; sh[r] = the offset
// of the row's first byte in its line, 0 for the rows of the tile that the image does not have
template <int RS>
__device__ __forceinline__ void fda_stage(uint8_t* raw, uint8_t* sh, const uint8_t* row0, long long pitch, int rows, int len, uintptr_t lo, uintptr_t hi, int t)
{
    constexpr int lpr = RS >> 4;
    for (int e = t; e < rows * lpr; e += FDA_THREADS) {
        const int r = e / lpr, i = e - r * lpr;
        const uintptr_t g = (uintptr_t)(row0 + (long long)r * pitch);
        const int shift = (int)(g & 15);
        if (i < ((shift + len + 15) >> 4)) *reinterpret_cast<uint4*>(raw + r * RS + 16 * i) = fda_fetch(lo, hi, g - shift + 16 * (uintptr_t)i);
    }
    if (t < FDA_RT) sh[t] = t < rows ? (uint8_t)((uintptr_t)(row0 + (long long)t * pitch) & 15) : (uint8_t)0;
}

// grid: (row tiles, N + M, pairs of column tiles).  G [N + M][H][3][CP]
__global__ __launch_bounds__(FDA_THREADS) void fda_rowdft_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ targets, int N, int M, int H, int W,
                                                                int b, const int* __restrict__ used, const float2* __restrict__ tww, float* __restrict__ G)
{
    __shared__ __attribute__((aligned(16))) uint8_t raw[FDA_RT * FDA_RS1];
    __shared__ float af[3 * FDA_KC * 32];                        // [channel][k][row]; at the end the other waves' sums, [wave - 1][register][lane]
    __shared__ uint8_t sh[FDA_RT];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int z = blockIdx.y;
    if (z >= N && !used[z - N]) return;                          // the whole block: a target no source refers to
    const long long P = (long long)H * W;
    const uint8_t* base = z < N ? images : targets;
    const uintptr_t lo = (uintptr_t)base, hi = lo + (uintptr_t)(z < N ? N : M) * (uintptr_t)P * 3;
    const uint8_t* img = base + (long long)(z < N ? z : z - N) * P * 3;
    const int h0 = blockIdx.x * FDA_RT, rows = min(FDA_RT, H - h0);
    const int CP = 2 * (b + 1), NT = (CP + 31) >> 5;             // NT <= 7
    const int nt0 = 2 * blockIdx.z, nq = min(2, NT - nt0);       // this block's column tiles: nt0 and, with nq = 2, nt0 + 1
    const int r = lane & 31, kh = lane >> 5;
    // the four waves deal the MFMA steps of a chunk among themselves: wave w takes the pixel pairs w, w + 4, ...; a lane's pixel advances by 8 per step
    int ph[2], inc[2], sn[2], ok[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int col = 32 * (nt0 + q) + r, v = min(col >> 1, b);
        ok[q] = col < CP; sn[q] = col & 1;
        ph[q] = (v * (2 * wave + kh)) % W;                       // (v w) mod W at the lane's first pixel
        inc[q] = (8 * v) % W;
    }
    fda_f32x16 acc[2][3];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[q][c][i] = 0.f;

    for (int w0 = 0; w0 < W; w0 += FDA_KC) {
        const int kw = min(FDA_KC, W - w0);
        fda_stage<FDA_RS1>(raw, sh, img + ((long long)h0 * W + w0) * 3, (long long)W * 3, rows, 3 * kw, lo, hi, t);
        __syncthreads();                                         // (and: every wave has left the previous chunk's multiplications)
        for (int e = t; e < 32 * 3 * FDA_KC; e += FDA_THREADS) {
            const int i = e & 31, jb = e >> 5, kk = jb / 3, c = jb - 3 * kk;
            af[(c * FDA_KC + kk) * 32 + i] = (i < rows && kk < kw) ? (float)raw[i * FDA_RS1 + sh[i] + jb] : 0.f;
        }
        __syncthreads();
        const int steps = (kw + 1) >> 1;                         // (a ragged chunk is the last one: the phases need not be stepped over its missing pixels)
        for (int s = wave; s < steps; s += 4) {
            const int kk = 2 * s + kh;
            const float a0 = af[kk * 32 + r], a1 = af[(FDA_KC + kk) * 32 + r], a2 = af[(2 * FDA_KC + kk) * 32 + r];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q < nq) {
                    const float2 tw = tww[ph[q]];
                    const float bv = ok[q] ? (sn[q] ? -tw.y : tw.x) : 0.f;
                    ph[q] += inc[q];
                    if (ph[q] >= W) ph[q] -= W;
                    acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[q][0], 0, 0, 0);
                    acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[q][1], 0, 0, 0);
                    acc[q][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, bv, acc[q][2], 0, 0, 0);
                }
            }
        }
    }
    // the four waves' sums meet in LDS, one accumulator at a time, and wave 0 adds them in wave order
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (q < nq) {                                            // block-uniform
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                __syncthreads();                                 // af is free: the multiplications, or the previous round's reads, are over
                if (wave) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) af[((wave - 1) * 16 + i) * 64 + lane] = acc[q][c][i];
                }
                __syncthreads();
                if (wave == 0 && ok[q]) {
                    const int col = 32 * (nt0 + q) + r;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
                        const float sum = ((acc[q][c][i] + af[i * 64 + lane]) + af[(16 + i) * 64 + lane]) + af[(32 + i) * 64 + lane];
                        if (row < rows) G[(((long long)z * H + h0 + row) * 3 + c) * CP + col] = sum;
                    }
                }
            }
        }
    }
}

// grid: (B * QCH, N + M), QCH = ceil(3 (b + 1) / 64).  F [N + M][B][3 (b + 1)] double2
__global__ __launch_bounds__(FDA_THREADS) void fda_coldft_kernel(int N, int H, int b, const int* __restrict__ used, const float2* __restrict__ twh,
                                                                const float* __restrict__ G, double2* __restrict__ F)
{
    __shared__ double2 red[FDA_THREADS];
    const int t = threadIdx.x, z = blockIdx.y;
    if (z >= N && !used[z - N]) return;
    const int Q = 3 * (b + 1), QCH = (Q + FDA_QW - 1) / FDA_QW, B = 2 * b + 1;
    const int ub = blockIdx.x / QCH, qc = blockIdx.x - ub * QCH;
    const int qw = min(FDA_QW, Q - qc * FDA_QW), NS = FDA_THREADS / qw;
    const int s = t / qw, q = qc * FDA_QW + (t - s * qw);
    const int um = ((ub - b) % H + H) % H;                       // u mod H
    double2 acc = make_double2(0.0, 0.0);
    if (s < NS) {
        int p = (int)(((long long)um * s) % H);
        const int inc = (int)(((long long)um * NS) % H);
        const float2* g = reinterpret_cast<const float2*>(G) + (long long)z * H * Q + q;
        for (int h = s; h < H; h += NS) {
            const float2 tw = twh[p], x = g[(long long)h * Q];
            p += inc;
            if (p >= H) p -= H;
            // e^{-i phi} (xr + i xi)
            acc.x = fma((double)tw.x, (double)x.x, fma((double)tw.y, (double)x.y, acc.x));
            acc.y = fma((double)tw.x, (double)x.y, fma(-(double)tw.y, (double)x.x, acc.y));
        }
    }
    red[t] = acc;
    __syncthreads();
    if (s == 0) {
        for (int k = 1; k < NS; ++k) { acc.x += red[k * qw + t].x; acc.y += red[k * qw + t].y; }
        F[((long long)z * B + ub) * Q + q] = acc;
    }
}

// one thread per (n, u, c, v).  D [N][B][3 (b + 1)] float2
__global__ __launch_bounds__(FDA_THREADS) void fda_delta_kernel(int N, int H, int W, int b, const int* __restrict__ pr, const double2* __restrict__ F,
                                                               float2* __restrict__ D)
{
    const int Q = 3 * (b + 1), B = 2 * b + 1;
    const long long per = (long long)B * Q, i = (long long)blockIdx.x * FDA_THREADS + threadIdx.x;
    if (i >= per * N) return;
    const int n = (int)(i / per);
    const long long e = i - (long long)n * per;
    const int v = (int)(e % Q) % (b + 1);
    const double2 fs = F[(long long)n * per + e], ft = F[(long long)(N + pr[n]) * per + e];
    const double a_s = sqrt(fs.x * fs.x + fs.y * fs.y), a_t = sqrt(ft.x * ft.x + ft.y * ft.y);
    const double k = (a_t - a_s) * ((v ? 2.0 : 1.0) / ((double)H * (double)W));
    const double px = a_s > 0.0 ? fs.x / a_s : 1.0, py = a_s > 0.0 ? fs.y / a_s : 0.0;
    D[i] = make_float2((float)(px * k), (float)(py * k));
}

// grid: (ceil(H / 4) * QCH, N); a wave owns one row h and 64 (c, v).  S [N][H][3][CP] over G
__global__ __launch_bounds__(FDA_THREADS) void fda_zsyn_kernel(int H, int b, const float2* __restrict__ twh, const float2* __restrict__ D, float* __restrict__ S)
{
    const int t = threadIdx.x, n = blockIdx.y;
    const int Q = 3 * (b + 1), QCH = (Q + FDA_QW - 1) / FDA_QW, B = 2 * b + 1;
    const int hb = blockIdx.x / QCH, qc = blockIdx.x - hb * QCH;
    const int h = hb * 4 + (t >> 6), q = qc * FDA_QW + (t & 63);
    if (h >= H || q >= Q) return;
    const int um = ((-b) % H + H) % H;
    int p = (int)(((long long)um * h) % H);
    const float2* d = D + (long long)n * B * Q + q;
    float zr = 0.f, zi = 0.f;
    for (int ub = 0; ub < B; ++ub) {
        const float2 tw = twh[p], x = d[(long long)ub * Q];
        p += h;                                                  // h < H
        if (p >= H) p -= H;
        zr = fmaf(tw.x, x.x, fmaf(-tw.y, x.y, zr));
        zi = fmaf(tw.x, x.y, fmaf(tw.y, x.x, zi));
    }
    reinterpret_cast<float2*>(S)[((long long)n * H + h) * Q + q] = make_float2(zr, -zi);
}

// grid: (tiles of 32 x 128 pixels, N)
__global__ __launch_bounds__(FDA_THREADS) void fda_synth_kernel(const uint8_t* __restrict__ images, int N, int H, int W, int b, int tiles_x,
                                                               const float2* __restrict__ tww, const float* __restrict__ S, uint8_t* __restrict__ out_u8,
                                                               float* __restrict__ out_f32)
{
    __shared__ __attribute__((aligned(16))) uint8_t raw[FDA_RT * FDA_RS2];
    __shared__ __attribute__((aligned(16))) uint8_t ob[FDA_RT * FDA_RS2];
    __shared__ float sl[3 * FDA_JC * 33];                        // [channel][j][row], rows 33 apart: the fill's lanes run along j
    __shared__ uint8_t ish[FDA_RT], osh[FDA_RT];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = blockIdx.y;
    const long long P = (long long)H * W;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * FDA_TW, y0 = ty * FDA_RT;
    const int tw_ = min(FDA_TW, W - x0), th = min(FDA_RT, H - y0);
    const int CP = 2 * (b + 1);
    const uint8_t* in0 = images + (long long)n * P * 3;
    const uintptr_t lo = (uintptr_t)images, hi = lo + (uintptr_t)N * (uintptr_t)P * 3;
    fda_stage<FDA_RS2>(raw, ish, in0 + ((long long)y0 * W + x0) * 3, (long long)W * 3, th, 3 * tw_, lo, hi, t);
    if (out_u8 && t < FDA_RT) osh[t] = t < th ? (uint8_t)((uintptr_t)(out_u8 + ((long long)n * P + (long long)(y0 + t) * W + x0) * 3) & 15) : (uint8_t)0;

    const int r = lane & 31, kh = lane >> 5;
    const int wx = min(x0 + 32 * wave + r, W - 1);               // a column past the edge computes what is never stored
    int ph = 0;                                                  // (v wx) mod W at v = 0
    fda_f32x16 acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
    const bool live = 32 * wave < tw_;                           // wave-uniform
    for (int j0 = 0; j0 < CP; j0 += FDA_JC) {
        const int jn = min(FDA_JC, CP - j0);                     // even
        __syncthreads();                                         // every wave has left the previous chunk (first trip: nothing)
        for (int e = t; e < 32 * 3 * FDA_JC; e += FDA_THREADS) {
            const int j = e % FDA_JC, rc = e / FDA_JC, c = rc % 3, i = rc / 3;
            sl[(c * FDA_JC + j) * 33 + i] = (i < th && j < jn) ? S[(((long long)n * H + y0 + i) * 3 + c) * CP + j0 + j] : 0.f;
        }
        __syncthreads();
        if (live) {
            for (int s = 0; s < (jn >> 1); ++s) {
                const int j = 2 * s + kh;
                const float2 tw = tww[ph];
                const float bv = kh ? tw.y : tw.x;
                ph += wx;
                if (ph >= W) ph -= W;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sl[j * 33 + r], bv, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(sl[(FDA_JC + j) * 33 + r], bv, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(sl[(2 * FDA_JC + j) * 33 + r], bv, acc[2], 0, 0, 0);
            }
        }
    }
    // (the staged bytes and the offsets are visible: the loop above has passed a barrier at least once, CP >= 2)
    const int px = 32 * wave + r;
    if (live && px < tw_) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
            if (row < th) {
                const uint8_t* s = raw + row * FDA_RS2 + ish[row] + 3 * px;
                const float y0f = (float)s[0] + acc[0][i], y1f = (float)s[1] + acc[1][i], y2f = (float)s[2] + acc[2][i];
                if (out_f32) {
                    float* o = out_f32 + ((long long)n * P + (long long)(y0 + row) * W + x0 + px) * 3;
                    o[0] = y0f; o[1] = y1f; o[2] = y2f;
                }
                if (out_u8) {
                    uint8_t* o = ob + row * FDA_RS2 + osh[row] + 3 * px;
                    o[0] = (uint8_t)fminf(fmaxf(rintf(y0f), 0.f), 255.f);
                    o[1] = (uint8_t)fminf(fmaxf(rintf(y1f), 0.f), 255.f);
                    o[2] = (uint8_t)fminf(fmaxf(rintf(y2f), 0.f), 255.f);
                }
            }
        }
    }
    if (!out_u8) return;                                         // block-uniform
    __syncthreads();
    // store: a line inside the row's bytes leaves as one 16-byte store, the ragged ones byte by byte
    {
        constexpr int lpr = FDA_RS2 >> 4;
        const int olen = 3 * tw_;
        uint8_t* out0 = out_u8 + (long long)n * P * 3;
        for (int e = t; e < th * lpr; e += FDA_THREADS) {
            const int rr = e / lpr, i = e - rr * lpr;
            const int shift = osh[rr], end = shift + olen, l0 = 16 * i;
            if (l0 >= end) continue;
            uint8_t* bs = out0 + ((long long)(y0 + rr) * W + x0) * 3 - shift;
            const uint8_t* s = ob + rr * FDA_RS2;
            if (l0 >= shift && l0 + 16 <= end) {
                *reinterpret_cast<uint4*>(bs + l0) = *reinterpret_cast<const uint4*>(s + l0);
            } else {
                const int j0 = l0 > shift ? l0 : shift, j1 = l0 + 16 < end ? l0 + 16 : end;
                for (int j = j0; j < j1; ++j) bs[j] = s[j];
            }
        }
    }
}

void launch_fda_transfer(const uint8_t* images, int N, const uint8_t* targets, int M, int H, int W, int b, const int* pair_dev, void* work, uint8_t* out_u8,
                         float* out_f32, hipStream_t s)
{
    const FdaLayout l = fda_layout(N, M, H, W, b);
    char* w0 = reinterpret_cast<char*>(((uintptr_t)work + 15) & ~(uintptr_t)15);
    unsigned int* flag = reinterpret_cast<unsigned int*>(w0);
    int* pr = reinterpret_cast<int*>(w0 + l.pr);
    int* used = reinterpret_cast<int*>(w0 + l.used);
    float2* tww = reinterpret_cast<float2*>(w0 + l.tww);
    float2* twh = reinterpret_cast<float2*>(w0 + l.twh);
    float* G = reinterpret_cast<float*>(w0 + l.g);
    double2* F = reinterpret_cast<double2*>(w0 + l.f);
    float2* D = reinterpret_cast<float2*>(w0 + l.d);
    const int Q = 3 * (b + 1), QCH = (Q + FDA_QW - 1) / FDA_QW, B = 2 * b + 1;
    const int big = H > W ? H : W;
    hipLaunchKernelGGL(fda_prep_kernel, dim3((big + FDA_THREADS - 1) / FDA_THREADS), dim3(FDA_THREADS), 0, s, N, M, H, W, pair_dev, flag, pr, used, tww, twh);
    hipLaunchKernelGGL(fda_rowdft_kernel, dim3((H + FDA_RT - 1) / FDA_RT, N + M, (b + 32) / 32), dim3(FDA_THREADS), 0, s, images, targets, N, M, H, W, b, used, tww, G);
    hipLaunchKernelGGL(fda_coldft_kernel, dim3(B * QCH, N + M), dim3(FDA_THREADS), 0, s, N, H, b, used, twh, G, F);
    const long long nd = (long long)N * B * Q;
    hipLaunchKernelGGL(fda_delta_kernel, dim3((unsigned)((nd + FDA_THREADS - 1) / FDA_THREADS)), dim3(FDA_THREADS), 0, s, N, H, W, b, pr, F, D);
    hipLaunchKernelGGL(fda_zsyn_kernel, dim3((unsigned)(((long long)H + 3) / 4 * QCH), N), dim3(FDA_THREADS), 0, s, H, b, twh, D, G);
    const int tiles_x = (W + FDA_TW - 1) / FDA_TW, tiles_y = (H + FDA_RT - 1) / FDA_RT;
    hipLaunchKernelGGL(fda_synth_kernel, dim3((unsigned)((long long)tiles_x * tiles_y), N), dim3(FDA_THREADS), 0, s, images, N, H, W, b, tiles_x, tww, G, out_u8,
                       out_f32);
}

}  // namespace fcn8s
