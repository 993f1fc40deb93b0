// Strong photometric augmentation (fcn8s_op_strong_augment; the definition is in fcn8s_hip.h): per image a gated colour jitter -- contrast about the
// image's mean grey, then saturation, brightness and hue in OpenCV's 8-bit HSV -- and a gated separable Gaussian blur with 11-bit integer taps and
// reflect-101 borders.  Integers plus the float32 steps of the 8-bit HSV -> RGB conversion: the device and strong_augment.py agree with ==.
//
// Up to three kernels, split at kernel boundaries as class_mix.hip is: no ticket, no fence, no block that waits for another, every loop bounded.
//   clear      zeroes the N grey sums in `work`.                                                       } launched only when the contrast
//   grey       sums g = (4899 R + 9617 G + 1868 B + 8192) >> 14 over every image whose colour gate      } strength is not 0
//              opens (the others leave at once).  A thread takes 16 pixels = 48 bytes as three 16-byte loads of whole lines plus the dword
//              behind them (a pixel may straddle the chunk's end; the phase of the pixels within a line is one of three per image and picks one
//              of three unrolled extractions); the pixels in front of the first line and behind the last whole chunk are read byte by byte by
//              block 0 of the image.  Integer adds only: a thread's sum, a wave's by shuffles, a block's in LDS, one 64-bit atomicAdd per block.
//   augment    reads the image once and writes it once.  A block owns a tile of SA_TH x SA_TW = 32 x 64 pixels of one image and stages it, with a
//              halo of R pixels where the image's blur gate is open (a block-uniform branch: an unblurred image pays for no halo), as raw bytes in
//              LDS: every row segment moves as whole 16-byte lines of global memory, a lane per line, and lies in LDS behind the offset its first
//              byte has in its line; a line that sticks out of the tensor is put together from its bytes inside.  The colour step runs on the
//              staged pixels, halo included (the neighbouring blocks recompute it: cheaper than a second trip through HBM), with the two
//              256-entry reciprocal tables of RGB2HSV_b built once per block in LDS instead of two double divisions per pixel.  Without a blur
//              it writes straight into the output strip.  Under a blur it writes an aligned copy -- pixel x0 - R of row y0 - R at byte 0 -- in
//              which every reflection is resolved once per pixel, not once per tap.  The horizontal pass gives a thread 4 pixels = 12 output
//              bytes of a row: output byte o is sum_t c[t] * (byte o + 3 t) with c[t] = w[|t - R|] (channel-blind: the neighbour of a byte lies
//              3 bytes away), so a register window of 12 + 6 R bytes, read as dwords, serves all twelve; the 20-bit sums go to a second LDS image
//              of SA_HS = 193 dwords per row (odd: the stores of neighbouring rows miss each other's banks), laid over the dead staged bytes.
//              The vertical pass puts the lanes along a row of it, so that 64 lanes read 64 consecutive dwords whatever the row stride, and
//              gives a thread 8 rows of a byte column from a window of 8 + 2 R sums.  (Measured at 16 x 1024 x 512, R = 4: 86 us against 216 us
//              with a byte fetch and two reflections per tap.)  The result is put together in the output strip behind the offset of the output
//              row and leaves as whole 16-byte lines, byte by byte at a row's ragged ends: no byte outside out_images is written.  The draws
//              (seven Philox words per image) are recomputed by every block; block 0 of an image writes params_out.
#include "fcn8s_internal.h"

namespace fcn8s {

#define SA_THREADS 256
#define SA_TW 64                                     // tile: pixels per row,
#define SA_TH 32                                     // rows
#define SA_OS 208                                    // output strip: 3 * SA_TW bytes behind an offset of 0 .. 15, in whole lines
#define SA_HS (3 * SA_TW + 1)                        // dwords per row of the horizontal sums: odd, so that the twelve stores of neighbouring rows miss each other's banks
#define SA_CS 236                                    // bytes per row of the aligned copy: 3 * (SA_TW + 14), and 59 dwords
#define SA_GREY_BLOCKS 2048                          // blocks of the grey grid over all images
#define SA_STREAM 0x53415547u                        // "SAUG"

// the host's small arrays, by value in the launch arguments: jitter {gate, Cs, Ss, Bs, Hs}, blur {gate, Q, R} (R = 0: no blur in this call)
struct SaArgs { int jitter[5]; int blur[3]; unsigned short taps[16][8]; };
struct SaDraw { int jit, contrast, hsv, c16, s16, b16, dh, blur, q; };

size_t strong_augment_work_bytes(int N) { return N > 0 ? 16 + (size_t)N * 8 : 0; }
__host__ __device__ static inline unsigned long long* sa_grey(void* work)
{
    return reinterpret_cast<unsigned long long*>(((uintptr_t)work + 15) & ~(uintptr_t)15);
}

// a uniform integer in [-S, S] from one word
__device__ __forceinline__ int sa_uniform(unsigned int u, int S)
{
    return -S + (int)(((unsigned long long)u * (unsigned long long)(2 * S + 1)) >> 32);
}
__device__ __forceinline__ bool sa_gate(unsigned int u, int gate) { return (int)(u >> 16) < gate; }

__device__ __forceinline__ SaDraw sa_draw(const SaArgs& a, int n, unsigned long long seed, unsigned long long draw)
{
    const unsigned long long c = (draw << 16) + ((unsigned long long)n << 8);
    SaDraw d = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    d.jit = sa_gate(philox_u32(c, seed, SA_STREAM), a.jitter[0]) ? 1 : 0;
    if (d.jit) {
        d.contrast = a.jitter[1] != 0;
        d.hsv = (a.jitter[2] | a.jitter[3] | a.jitter[4]) != 0;
        if (d.contrast) d.c16 = 65536 + sa_uniform(philox_u32(c + 1, seed, SA_STREAM), a.jitter[1]);
        if (d.hsv) {
            d.s16 = 65536 + sa_uniform(philox_u32(c + 2, seed, SA_STREAM), a.jitter[2]);
            d.b16 = 65536 + sa_uniform(philox_u32(c + 3, seed, SA_STREAM), a.jitter[3]);
            d.dh = sa_uniform(philox_u32(c + 4, seed, SA_STREAM), a.jitter[4]);
        }
    }
    d.blur = (a.blur[2] > 0 && sa_gate(philox_u32(c + 5, seed, SA_STREAM), a.blur[0])) ? 1 : 0;
    if (d.blur) d.q = (int)(((unsigned long long)philox_u32(c + 6, seed, SA_STREAM) * (unsigned long long)a.blur[1]) >> 32);
    return d;
}

__global__ __launch_bounds__(SA_THREADS) void strong_augment_clear_kernel(unsigned long long* grey, int N)
{
    const int i = blockIdx.x * SA_THREADS + threadIdx.x;
    if (i < N) grey[i] = 0ull;
}

__device__ __forceinline__ unsigned int sa_grey_of(unsigned int r, unsigned int g, unsigned int b)
{
    return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;
}
// the 16 pixels that begin S bytes behind the start of a window of 13 dwords
template <int S>
__device__ __forceinline__ unsigned int sa_grey16(const unsigned int* w)
{
    unsigned int sum = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int o = S + 3 * i;
        sum += sa_grey_of((w[o >> 2] >> (8 * (o & 3))) & 255u, (w[(o + 1) >> 2] >> (8 * ((o + 1) & 3))) & 255u, (w[(o + 2) >> 2] >> (8 * ((o + 2) & 3))) & 255u);
    }
    return sum;
}

// grid: (blocks per image, N)
__global__ __launch_bounds__(SA_THREADS) void strong_augment_grey_kernel(const uint8_t* __restrict__ images, long long P, unsigned long long seed,
                                                                        unsigned long long draw, int gate, unsigned long long* grey)
{
    __shared__ unsigned long long part[SA_THREADS / 64];
    const int t = threadIdx.x, n = blockIdx.y;
    if (!sa_gate(philox_u32((draw << 16) + ((unsigned long long)n << 8), seed, SA_STREAM), gate)) return;      // the whole block: no colour step, no mean
    const uint8_t* b = images + (long long)n * P * 3;
    const long long bytes = P * 3;
    const int head = (int)((16 - ((uintptr_t)b & 15)) & 15);                                    // bytes in front of the first whole line
    const long long nchunk = bytes - head - 4 >= 48 ? (bytes - head - 4) / 48 : 0;              // chunks of 48 bytes whose 52-byte window lies inside the image
    long long p_head = (head + 2) / 3;                                                          // pixels that begin in front of the first line
    if (p_head > P) p_head = P;
    const int s = (int)(3 * p_head - head);                                                     // where the first pixel of a chunk begins: 0, 1 or 2 (unused without chunks)
    const long long p_tail = nchunk ? p_head + 16 * nchunk : p_head;
    const uint8_t* a = b + head;
    unsigned long long sum = 0ull;
    for (long long k = (long long)blockIdx.x * SA_THREADS + t; k < nchunk; k += (long long)gridDim.x * SA_THREADS) {
        const uint4* v = reinterpret_cast<const uint4*>(a + 48 * k);
        const uint4 q0 = v[0], q1 = v[1], q2 = v[2];
        const unsigned int w[13] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, *reinterpret_cast<const unsigned int*>(v + 3)};
        sum += s == 0 ? sa_grey16<0>(w) : (s == 1 ? sa_grey16<1>(w) : sa_grey16<2>(w));
    }
    if (blockIdx.x == 0) {                           // the ragged ends: at most 5 pixels in front and fewer than 40 behind
        const long long ends = p_head + (P - p_tail);
        for (long long i = t; i < ends; i += SA_THREADS) {
            const long long p = i < p_head ? i : p_tail + (i - p_head);
            sum += sa_grey_of(b[3 * p], b[3 * p + 1], b[3 * p + 2]);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
    if ((t & 63) == 0) part[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long all = 0ull;
        for (int i = 0; i < SA_THREADS / 64; ++i) all += part[i];
        if (all) atomicAdd(&grey[n], all);
    }
}

// OpenCV's 8-bit RGB <-> HSV (H in [0, 180)) as elementwise.hip and cv2_compat.py define them, restated with RGB2HSV_b's two reciprocal tables
// (sdiv[v] = cvRound((255 << 12) / v), hdiv[d] = cvRound((180 << 12) / (6 d))) read from LDS.  The float steps use the *_rn intrinsics so that
// the compiler cannot contract a multiply and a subtract into one FMA.
__device__ __forceinline__ void sa_rgb2hsv(int r, int g, int b, const int* sdiv, const int* hdiv, int& h, int& s, int& v)
{
    v = max(max(r, g), b);
    const int vmin = min(min(r, g), b), diff = v - vmin;
    s = (diff * sdiv[v] + (1 << 11)) >> 12;
    int hh = v == r ? (g - b) : (v == g ? (b - r + 2 * diff) : (r - g + 4 * diff));
    hh = (hh * hdiv[diff] + (1 << 11)) >> 12;
    h = hh < 0 ? hh + 180 : hh;
}
__device__ __forceinline__ int sa_sat(float x)
{
    const int q = (int)rintf(__fmul_rn(x, 255.f));
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}
__device__ __forceinline__ void sa_hsv2rgb(int H, int S, int V, int& r, int& g, int& b)
{
    const float s = __fmul_rn((float)S, 1.f / 255.f), v = __fmul_rn((float)V, 1.f / 255.f);
    float fb, fg, fr;
    if (s == 0.f) fb = fg = fr = v;
    else {
        float h = __fmul_rn((float)H, 6.f / 180.f);
        if (h >= 6.f) h = __fsub_rn(h, 6.f);
        int sector = (int)floorf(h);
        h = __fsub_rn(h, (float)sector);
        if ((unsigned)sector >= 6u) { sector = 0; h = 0.f; }
        const float t0 = v, t1 = __fmul_rn(v, __fsub_rn(1.f, s)), t2 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, h))),
                    t3 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, __fsub_rn(1.f, h))));
        switch (sector) {                      // sector_data: tab index of (b, g, r)
            case 0:  fb = t1; fg = t3; fr = t0; break;
            case 1:  fb = t1; fg = t0; fr = t2; break;
            case 2:  fb = t3; fg = t0; fr = t1; break;
            case 3:  fb = t0; fg = t2; fr = t1; break;
            case 4:  fb = t0; fg = t1; fr = t3; break;
            default: fb = t2; fg = t1; fr = t0; break;
        }
    }
    r = sa_sat(fr); g = sa_sat(fg); b = sa_sat(fb);
}

// the colour step of one pixel
__device__ __forceinline__ void sa_colour(const SaDraw& d, int m, const int* sdiv, const int* hdiv, int& r, int& g, int& b)
{
    if (d.contrast) {
        const int k = m * (65536 - d.c16) + 32768;
        r = min(max((r * d.c16 + k) >> 16, 0), 255);
        g = min(max((g * d.c16 + k) >> 16, 0), 255);
        b = min(max((b * d.c16 + k) >> 16, 0), 255);
    }
    if (d.hsv) {
        int h, s, v;
        sa_rgb2hsv(r, g, b, sdiv, hdiv, h, s, v);
        h = (h + 180 + d.dh) % 180;
        s = min(255, (s * d.s16 + 32768) >> 16);
        v = min(255, (v * d.b16 + 32768) >> 16);
        sa_hsv2rgb(h, s, v, r, g, b);
    }
}

// the 16-byte line of global memory at g; where it sticks out of the tensor [lo, hi), its bytes inside
__device__ __forceinline__ uint4 sa_fetch(uintptr_t lo, uintptr_t hi, uintptr_t g)
{
    if (g >= lo && g + 16 <= hi) return *reinterpret_cast<const uint4*>(g);
    unsigned int w[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < 16; ++j)
        if (g + j >= lo && g + j < hi) w[j >> 2] |= (unsigned int)*reinterpret_cast<const uint8_t*>(g + j) << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ int sa_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// the LDS of the augment kernel, by the radius R of the call's blur (0: no blur in this call): region A holds the staged bytes [rows][RS] and, once
// they are dead, the horizontal sums [rows][SA_HS]; then the output strip, the two tables, the coefficients and the rows' offsets; then the aligned
// copy [rows][SA_CS] that the blur reads
struct SaLds { int rs, a_bytes, cb_bytes, total; };
__host__ __device__ static inline SaLds sa_lds(int R)
{
    const int rows = SA_TH + 2 * R;
    SaLds l;
    l.rs = ((15 + 3 * (SA_TW + 2 * R) + 15) / 16) * 16;
    const int raw = rows * l.rs, hs = R ? rows * SA_HS * 4 : 0;
    l.a_bytes = ((raw > hs ? raw : hs) + 15) & ~15;
    l.cb_bytes = R ? (rows * SA_CS + 15) & ~15 : 0;
    l.total = l.a_bytes + SA_TH * SA_OS + 2048 + 64 + 48 + 32 + l.cb_bytes;             // at most 55232 bytes (R = 7)
    return l;
}

// byte b of a window of dwords (b is a constant after unrolling)
#define SA_BYTE(win, b) (((win)[(b) >> 2] >> (8 * ((b) & 3))) & 255u)

// grid: (tiles of an image, N); dynamic LDS: sa_lds(R).total
__global__ __launch_bounds__(SA_THREADS) void strong_augment_kernel(const uint8_t* __restrict__ images, int N, int H, int W, int tiles_x, unsigned long long seed,
                                                                   unsigned long long draw, SaArgs a, const unsigned long long* __restrict__ grey,
                                                                   uint8_t* __restrict__ out, int* __restrict__ params_out)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x, n = blockIdx.y;
    const SaLds l = sa_lds(a.blur[2]);
    const int RS = l.rs;
    uint8_t* raw = lds;                                                  // [rows][RS]: the staged bytes, a row behind the offset ish[row]
    unsigned int* hs = reinterpret_cast<unsigned int*>(lds);             // [th + 2 R][SA_HS]: the horizontal sums, over the dead staged bytes
    uint8_t* ob = lds + l.a_bytes;                                       // [SA_TH][SA_OS]: the output rows, a row behind the offset osh[row]
    int* sdiv = reinterpret_cast<int*>(ob + SA_TH * SA_OS);
    int* hdiv = sdiv + 256;
    unsigned int* cw = reinterpret_cast<unsigned int*>(hdiv + 256);      // [16]: c[t] = w[|t - R|] for t <= 2 R, 0 behind
    uint8_t* ish = reinterpret_cast<uint8_t*>(cw + 16);                  // [48]
    uint8_t* osh = ish + 48;                                             // [32]
    uint8_t* cb = osh + 32;                                              // [th + 2 R][SA_CS]: pixels x0 - R .. x0 + tw + R - 1 of rows y0 - R .. y0 + th + R - 1,
                                                                         // reflected at the image's borders, after the colour step, from byte 0 of a row
    const SaDraw d = sa_draw(a, n, seed, draw);
    const long long P = (long long)H * W;
    int m = 0;
    if (d.contrast) m = (int)((2ull * grey[n] + (unsigned long long)P) / (2ull * (unsigned long long)P));
    if (params_out && blockIdx.x == 0 && t == 0) {
        int* po = params_out + n * 8;
        po[0] = d.jit; po[1] = d.c16; po[2] = d.s16; po[3] = d.b16; po[4] = d.dh; po[5] = m; po[6] = d.blur; po[7] = d.q;
    }
    const int R = d.blur ? a.blur[2] : 0;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * SA_TW, y0 = ty * SA_TH;
    const int tw = min(SA_TW, W - x0), th = min(SA_TH, H - y0);
    const int xs = max(0, x0 - R), xe = min(W, x0 + tw + R), ys = max(0, y0 - R), ye = min(H, y0 + th + R);
    const int rows = ye - ys, seg = xe - xs, len = 3 * seg;              // rows <= SA_TH + 2 R, 15 + len <= RS
    const uint8_t* in0 = images + (long long)n * P * 3;
    uint8_t* out0 = out + (long long)n * P * 3;

    // stage: whole lines, a lane per line
    {
        const uintptr_t lo = (uintptr_t)images, hi = lo + (uintptr_t)N * (uintptr_t)P * 3;
        const int lpr = RS >> 4;
        for (int e = t; e < rows * lpr; e += SA_THREADS) {
            const int r = e / lpr, i = e - r * lpr;
            const uintptr_t g = (uintptr_t)(in0 + ((long long)(ys + r) * W + xs) * 3);
            const int shift = (int)(g & 15);
            if (i < ((shift + len + 15) >> 4)) *reinterpret_cast<uint4*>(raw + r * RS + 16 * i) = sa_fetch(lo, hi, g - shift + 16 * (uintptr_t)i);
        }
        if (t < rows) ish[t] = (uint8_t)((uintptr_t)(in0 + ((long long)(ys + t) * W + xs) * 3) & 15);
        if (t < th) osh[t] = (uint8_t)((uintptr_t)(out0 + ((long long)(y0 + t) * W + x0) * 3) & 15);
        if (d.hsv) {
            sdiv[t] = t ? (int)rint((double)(255 << 12) / (double)t) : 0;
            hdiv[t] = t ? (int)rint((double)(180 << 12) / (6.0 * (double)t)) : 0;
        }
        if (d.blur && t < 16) cw[t] = t <= 2 * R ? a.taps[d.q][t < R ? R - t : t - R] : 0u;
    }
    __syncthreads();

    if (!d.blur) {                                                       // block-uniform: no halo was staged (xs = x0, ys = y0)
        if (d.contrast | d.hsv) {
            for (int e = t; e < th * tw; e += SA_THREADS) {
                const int r = e / tw, px = e - r * tw;
                const uint8_t* s = raw + r * RS + ish[r] + 3 * px;
                int cr = s[0], cg = s[1], cb_ = s[2];
                sa_colour(d, m, sdiv, hdiv, cr, cg, cb_);
                uint8_t* o = ob + r * SA_OS + osh[r] + 3 * px;
                o[0] = (uint8_t)cr; o[1] = (uint8_t)cg; o[2] = (uint8_t)cb_;
            }
        } else {
            for (int e = t; e < th * 3 * tw; e += SA_THREADS) {
                const int r = e / (3 * tw), j = e - r * 3 * tw;
                ob[r * SA_OS + osh[r] + j] = raw[r * RS + ish[r] + j];
            }
        }
        __syncthreads();
    } else {
        // the colour step (or a plain move) into the aligned copy, where every reflection is resolved once per pixel, not once per tap
        const int bw = tw + 2 * R, bh = th + 2 * R;
        for (int e = t; e < bh * bw; e += SA_THREADS) {
            const int r = e / bw, p = e - r * bw;
            const int y = sa_reflect(y0 - R + r, H) - ys, x = sa_reflect(x0 - R + p, W) - xs;
            const uint8_t* s = raw + y * RS + ish[y] + 3 * x;
            int cr = s[0], cg = s[1], cb_ = s[2];
            if (d.contrast | d.hsv) sa_colour(d, m, sdiv, hdiv, cr, cg, cb_);
            uint8_t* o = cb + r * SA_CS + 3 * p;
            o[0] = (uint8_t)cr; o[1] = (uint8_t)cg; o[2] = (uint8_t)cb_;
        }
        __syncthreads();                                                 // the staged bytes are dead: hs may overwrite them

        unsigned int c[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) c[i] = cw[i];
        // horizontal: a thread takes 4 pixels = 12 output bytes of one row: output byte o is sum_t c[t] * (byte o + 3 t of the aligned copy), so a
        // window of 12 + 6 R bytes, read as dwords (a group begins at byte 12 g of its row), serves all twelve
        {
            const int groups = (tw + 3) >> 2;
            const unsigned int* cbw = reinterpret_cast<const unsigned int*>(cb);
            for (int e = t; e < bh * groups; e += SA_THREADS) {
                const int r = e / groups, g = e - r * groups;
                const unsigned int* src = cbw + r * (SA_CS / 4) + 3 * g;
                unsigned int win[14];
#pragma unroll
                for (int k = 0; k < 14; ++k) win[k] = 4 * k < 12 + 6 * R ? src[k] : 0u;
                unsigned int acc[12];
#pragma unroll
                for (int o = 0; o < 12; ++o) acc[o] = c[0] * SA_BYTE(win, o);
#pragma unroll
                for (int i = 1; i < 15; ++i) {
                    if (i <= 2 * R) {
#pragma unroll
                        for (int o = 0; o < 12; ++o) acc[o] += c[i] * SA_BYTE(win, o + 3 * i);
                    }
                }
                unsigned int* dst = hs + r * SA_HS + 12 * g;
#pragma unroll
                for (int o = 0; o < 12; ++o) dst[o] = acc[o];
            }
        }
        __syncthreads();
        // vertical: lanes along a row of dwords; a thread takes 8 rows of one byte column from a window of 8 + 2 R sums
        {
            const int runs = (th + 7) >> 3, cols = 3 * tw;
            for (int e = t; e < runs * cols; e += SA_THREADS) {
                const int run = e / cols, j = e - run * cols;
                const unsigned int* src = hs + (8 * run) * SA_HS + j;
                unsigned int win[22];
#pragma unroll
                for (int k = 0; k < 22; ++k) win[k] = k < 8 + 2 * R ? src[k * SA_HS] : 0u;
                unsigned int acc[8];
#pragma unroll
                for (int o = 0; o < 8; ++o) acc[o] = c[0] * win[o];
#pragma unroll
                for (int i = 1; i < 15; ++i) {
                    if (i <= 2 * R) {
#pragma unroll
                        for (int o = 0; o < 8; ++o) acc[o] += c[i] * win[o + i];
                    }
                }
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const int r = 8 * run + o;
                    if (r < th) ob[r * SA_OS + osh[r] + j] = (uint8_t)((acc[o] + (1u << 21)) >> 22);
                }
            }
        }
        __syncthreads();
    }

    // store: a line inside the row's bytes leaves as one 16-byte store, the ragged ones byte by byte
    {
        const int lpr = SA_OS >> 4, olen = 3 * tw;
        for (int e = t; e < th * lpr; e += SA_THREADS) {
            const int r = e / lpr, i = e - r * lpr;
            const int shift = osh[r], end = shift + olen, l0 = 16 * i;
            if (l0 >= end) continue;
            uint8_t* base = out0 + ((long long)(y0 + r) * W + x0) * 3 - shift;
            const uint8_t* s = ob + r * SA_OS;
            if (l0 >= shift && l0 + 16 <= end) {
                *reinterpret_cast<uint4*>(base + l0) = *reinterpret_cast<const uint4*>(s + l0);
            } else {
                const int j0 = l0 > shift ? l0 : shift, j1 = l0 + 16 < end ? l0 + 16 : end;
                for (int j = j0; j < j1; ++j) base[j] = s[j];
            }
        }
    }
}

void launch_strong_augment(const uint8_t* images, int N, int H, int W, unsigned long long seed, unsigned long long draw, const int* jitter, const int* blur,
                           const unsigned short* taps, void* work, uint8_t* out_images, int* params_out, hipStream_t s)
{
    SaArgs a = {};
    if (jitter) for (int i = 0; i < 5; ++i) a.jitter[i] = jitter[i];
    a.blur[1] = 1;
    if (blur) {
        for (int i = 0; i < 3; ++i) a.blur[i] = blur[i];
        for (int q = 0; q < blur[1]; ++q)
            for (int i = 0; i <= blur[2]; ++i) a.taps[q][i] = taps[q * (blur[2] + 1) + i];
    }
    unsigned long long* grey = sa_grey(work);
    const long long P = (long long)H * W;
    if (a.jitter[0] > 0 && a.jitter[1] != 0) {
        hipLaunchKernelGGL(strong_augment_clear_kernel, dim3((N + SA_THREADS - 1) / SA_THREADS), dim3(SA_THREADS), 0, s, grey, N);
        const long long per_image = (SA_GREY_BLOCKS + N - 1) / N, chunks = (P * 3 + 47) / 48, blocks = (chunks + SA_THREADS - 1) / SA_THREADS;
        hipLaunchKernelGGL(strong_augment_grey_kernel, dim3((unsigned)(blocks < per_image ? blocks : per_image), N), dim3(SA_THREADS), 0, s, images, P, seed, draw,
                           a.jitter[0], grey);
    }
    const int tiles_x = (W + SA_TW - 1) / SA_TW, tiles_y = (H + SA_TH - 1) / SA_TH;
    hipLaunchKernelGGL(strong_augment_kernel, dim3((unsigned)((long long)tiles_x * tiles_y), N), dim3(SA_THREADS), (size_t)sa_lds(a.blur[2]).total, s, images, N, H, W,
                       tiles_x, seed, draw, a, grey, out_images, params_out);
}

}  // namespace fcn8s
