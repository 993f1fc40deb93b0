// ClassMix (fcn8s_op_class_mix; the definition is in fcn8s_hip.h): half of the classes present in a source image are cut out along its label
// mask and pasted onto a destination image, pixels and labels alike.  Integers only: ORs and compares decide everything.
//
// Four kernels, split at kernel boundaries as regions.hip and panoptic.hip are: no ticket, no fence, no block that waits for another, every loop
// bounded.
//   clear      zeroes the per-image presence sets (8 words each) and the flag word.
//   presence   reads every label byte once.  A block belongs to one image (blockIdx.y) and walks its 16-byte lines with lane-contiguous loads, four
//              in flight per thread (measured at 16 x 1024 x 512: 7.8 us against 9.3 us with one load per trip and four times the blocks); the
//              bytes in front of the first and behind the last whole line (any alignment of labels + n P) are read one by one by block 0 of the
//              image.  A thread keeps the classes below 64 in a 64-bit register set -- no atomic at all for C <= 64 -- and sends a class from
//              64 on to the block's LDS set with one OR whenever it differs from the one it met before.  The waves OR their register sets
//              together (six DPP / permute steps), one lane per wave ORs the result into LDS, and the block ends with one global 32-bit
//              atomicOr per non-zero word.
//   selection  one block of 256 threads per destination image: thread c computes key(c) with the library's Philox, the ranks are counted over the
//              keys in LDS (C broadcast reads per thread), and the 256-byte table goes to `work` and, unless it is NULL, to selected_out.
//   mix        streams 12 bytes per pixel: 4 read from each of the two images and their labels, 4 written.  A block takes tiles of CM_TILE = 1024
//              pixels of one image: 1 KiB of labels and 3 KiB of RGB per stream.  Every stream is moved in whole 16-byte lines of GLOBAL memory,
//              a lane per line, so that a wave's access is 1 KiB of consecutive bytes whatever the pointers' alignment: a stream's tile is
//              staged in LDS behind the offset (0 .. 15) that its first byte has inside its line.  A thread's four loads of a tile are issued
//              together into registers, and the next tile's while the current one is mixed and stored.  A line that sticks out of the array (loads)
//              or out of the tile (stores) is moved byte by byte, and no byte outside the N P (3 N P) bytes of an output is written.  Between
//              the two, thread t mixes the pixels 4 t .. 4 t + 3: the 3-byte pixels are regrouped through LDS, not by striding 48 bytes between
//              lanes.  Where all six offsets are multiples of 4 (always, for 16-byte aligned tensors and P % 4 == 0) it moves dwords -- one
//              of labels and three of RGB per stream, at an odd dword stride, so that 32 lanes meet 32 banks -- and selects with byte masks;
//              otherwise it moves bytes.  The table (256 bytes = 64 dwords) is in LDS; it is 0 for every id >= C, so no compare is needed.
#include "fcn8s_internal.h"

namespace fcn8s {

#define CM_THREADS 256
#define CM_TILE 1024                                 // pixels per tile: 4 per thread
#define CM_LSTRIP (CM_TILE + 16)                     // a tile of labels behind an offset of 0 .. 15 bytes
#define CM_ISTRIP (3 * CM_TILE + 16)
#define CM_BLOCKS 2048                               // blocks of the presence and mix grids, over all images (256 CUs x 8 blocks of 4 waves)
#define CM_PRESENCE_LOADS 4                          // 16-byte loads a thread of the presence kernel has in flight
#define CM_STREAM 0x434D4958u                        // "CMIX"

// `work` behind its first 16-byte boundary: presence [N][8] uint32, table [N][256] uint8, flag [4] uint32
struct CmWork { unsigned int* presence; uint8_t* table; unsigned int* flag; };
__host__ __device__ static inline CmWork cm_work(void* work, int N)
{
    uint8_t* b = reinterpret_cast<uint8_t*>(((uintptr_t)work + 15) & ~(uintptr_t)15);
    CmWork w;
    w.presence = reinterpret_cast<unsigned int*>(b);
    w.table = b + (size_t)N * 32;
    w.flag = reinterpret_cast<unsigned int*>(b + (size_t)N * 288);
    return w;
}
size_t class_mix_work_bytes(int N) { return N > 0 ? 16 + (size_t)N * 288 + 16 : 0; }

__global__ __launch_bounds__(CM_THREADS) void class_mix_clear_kernel(unsigned int* presence, unsigned int* flag, int words)
{
    const int i = blockIdx.x * CM_THREADS + threadIdx.x;
    if (i < words) presence[i] = 0u;
    if (i < 4) flag[i] = 0u;
}

// one label byte into the thread's sets
__device__ __forceinline__ void cm_see(unsigned int c, unsigned int C, unsigned long long& low, unsigned int& last, unsigned int* set)
{
    if (c < C) {
        if (c < 64u) low |= 1ull << c;
        else if (c != last) { atomicOr(&set[c >> 5], 1u << (c & 31u)); last = c; }
    }
}

// grid: (blocks per image, N)
__global__ __launch_bounds__(CM_THREADS) void class_mix_presence_kernel(const uint8_t* __restrict__ labels, long long P, unsigned int C, unsigned int* presence)
{
    __shared__ unsigned int set[8];
    const int t = threadIdx.x, n = blockIdx.y;
    if (t < 8) set[t] = 0u;
    __syncthreads();
    const uint8_t* lp = labels + (long long)n * P;
    long long head = (long long)((16 - ((uintptr_t)lp & 15)) & 15);
    if (head > P) head = P;
    const long long nvec = (P - head) >> 4, tail0 = head + (nvec << 4);
    const uint4* vp = reinterpret_cast<const uint4*>(lp + head);
    unsigned long long low = 0ull;
    unsigned int last = 0xFFFFFFFFu;
    const long long stride = (long long)gridDim.x * CM_THREADS;
    for (long long i = (long long)blockIdx.x * CM_THREADS + t; i < nvec; i += CM_PRESENCE_LOADS * stride) {
        uint4 q[CM_PRESENCE_LOADS];                                                             // all in flight before the first is looked at
#pragma unroll
        for (int u = 0; u < CM_PRESENCE_LOADS; ++u) q[u] = i + u * stride < nvec ? vp[i + u * stride] : make_uint4(~0u, ~0u, ~0u, ~0u);      // 255: no class
#pragma unroll
        for (int u = 0; u < CM_PRESENCE_LOADS; ++u) {
            const unsigned int w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int b = 0; b < 4; ++b) cm_see((w[j] >> (8 * b)) & 255u, C, low, last, set);
            }
        }
    }
    if (blockIdx.x == 0) {                           // the ragged ends: fewer than 16 bytes each
        if (t < head) cm_see(lp[t], C, low, last, set);
        if (t >= 16 && tail0 + (t - 16) < P) cm_see(lp[tail0 + (t - 16)], C, low, last, set);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) low |= (unsigned long long)__shfl_xor((long long)low, d, 64);
    if ((t & 63) == 0) {
        if ((unsigned int)low) atomicOr(&set[0], (unsigned int)low);
        if ((unsigned int)(low >> 32)) atomicOr(&set[1], (unsigned int)(low >> 32));
    }
    __syncthreads();
    if (t < 8 && set[t]) atomicOr(&presence[n * 8 + t], set[t]);
}

// src[n], or n when it lies outside [0, N)
__device__ __forceinline__ int cm_source(const int* src, int n, int N, bool& bad)
{
    const int s = src[n];
    bad = s < 0 || s >= N;
    return bad ? n : s;
}

// grid: N, block: 256
__global__ __launch_bounds__(CM_THREADS) void class_mix_select_kernel(const int* __restrict__ src, int N, int C, unsigned long long seed, unsigned long long draw,
                                                                     CmWork w, uint8_t* selected_out)
{
    __shared__ unsigned int key[256];
    __shared__ unsigned int here[256];
    const int c = threadIdx.x, n = blockIdx.x;
    bool bad;
    const int s = cm_source(src, n, N, bad);
    if (bad && c == 0) atomicOr(w.flag, 1u);
    const unsigned int on = c < C ? (w.presence[s * 8 + (c >> 5)] >> (c & 31)) & 1u : 0u;
    const unsigned int k = philox_u32((draw << 16) + ((unsigned long long)n << 8) + (unsigned long long)c, seed, CM_STREAM);
    key[c] = k; here[c] = on;
    __syncthreads();
    int present = 0, rank = 0;
    for (int o = 0; o < C; ++o) {
        if (here[o]) {
            ++present;
            const unsigned int ko = key[o];
            if (ko < k || (ko == k && o < c)) ++rank;
        }
    }
    const uint8_t sel = (on && rank < (present + 1) / 2) ? 1 : 0;
    w.table[n * 256 + c] = sel;
    if (selected_out) selected_out[n * 256 + c] = sel;
}

// Line i of the tile's bytes [p, p + len) of an array [lo, hi): the 16-byte line of global memory at (p & ~15) + 16 i, which cm_put stores at
// lds + 16 i, so that the tile lies in lds behind the offset p & 15.  A line that is not wholly inside the array is put together from its bytes
// inside it.  Registers only: a tile is fetched while the one before it is still in LDS.
__device__ __forceinline__ uint4 cm_fetch(const uint8_t* lo, const uint8_t* hi, const uint8_t* p, int len, int i)
{
    const int shift = (int)((uintptr_t)p & 15), nlines = (shift + len + 15) >> 4;
    const uintptr_t a = (uintptr_t)lo, b = (uintptr_t)hi, g = (uintptr_t)p - shift + (uintptr_t)i * 16;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i < nlines) {
        if (g >= a && g + 16 <= b) {
            v = *reinterpret_cast<const uint4*>(g);
        } else {
            unsigned int w[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; j < 16; ++j)
                if (g + j >= a && g + j < b) w[j >> 2] |= (unsigned int)*reinterpret_cast<const uint8_t*>(g + j) << (8 * (j & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    return v;
}
__device__ __forceinline__ void cm_put(const uint4& v, uint8_t* lds, int i, int lines)
{
    if (i < lines) *reinterpret_cast<uint4*>(lds + i * 16) = v;
}

// what a thread holds of a tile before it is in LDS: one line of each input stream (the source's labels go to the threads from the first
// one up, the destination's from the last one down)
struct CmTile { uint4 ls, ln, is, in; };
__device__ __forceinline__ CmTile cm_fetch_tile(const uint8_t* images, const uint8_t* labels, int s, int n, int N, long long P, long long tile, int t)
{
    const long long p0 = tile * CM_TILE;
    const int npx = P - p0 < CM_TILE ? (int)(P - p0) : CM_TILE;
    const uint8_t* lab_end = labels + (long long)N * P;
    const uint8_t* img_end = images + (long long)N * P * 3;
    CmTile r;
    r.ls = cm_fetch(labels, lab_end, labels + (long long)s * P + p0, npx, t);
    r.ln = cm_fetch(labels, lab_end, labels + (long long)n * P + p0, npx, CM_THREADS - 1 - t);
    r.is = cm_fetch(images, img_end, images + ((long long)s * P + p0) * 3, 3 * npx, t);
    r.in = cm_fetch(images, img_end, images + ((long long)n * P + p0) * 3, 3 * npx, t);
    return r;
}

// lds, behind the offset p & 15, into the tile's bytes [p, p + len): a line that lies inside the tile leaves as one 16-byte store, the ragged
// ones as byte stores of their bytes inside the tile
__device__ __forceinline__ void cm_store_lines(uint8_t* p, int len, const uint8_t* lds, int t)
{
    const int shift = (int)((uintptr_t)p & 15), end = shift + len, nlines = (end + 15) >> 4;
    uint8_t* base = p - shift;
    for (int i = t; i < nlines; i += CM_THREADS) {
        const int l0 = i * 16;
        if (l0 >= shift && l0 + 16 <= end) {
            *reinterpret_cast<uint4*>(base + l0) = *reinterpret_cast<const uint4*>(lds + l0);
        } else {
            const int j0 = l0 > shift ? l0 : shift, j1 = l0 + 16 < end ? l0 + 16 : end;
            for (int j = j0; j < j1; ++j) base[j] = lds[j];
        }
    }
}

// grid: (blocks per image, N)
__global__ __launch_bounds__(CM_THREADS) void class_mix_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ labels, const int* __restrict__ src,
                                                              int N, long long P, const uint8_t* table, uint8_t* __restrict__ out_images,
                                                              uint8_t* __restrict__ out_labels)
{
    __shared__ __attribute__((aligned(16))) uint8_t ls[CM_LSTRIP], ln[CM_LSTRIP], lo[CM_LSTRIP];
    __shared__ __attribute__((aligned(16))) uint8_t is[CM_ISTRIP], in[CM_ISTRIP], io[CM_ISTRIP];
    __shared__ __attribute__((aligned(16))) uint8_t tab[256];
    const int t = threadIdx.x, n = blockIdx.y;
    bool bad;
    const int s = cm_source(src, n, N, bad);
    tab[t] = table[n * 256 + t];
    const long long tiles = (P + CM_TILE - 1) / CM_TILE;
    CmTile r = cm_fetch_tile(images, labels, s, n, N, P, blockIdx.x, t);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = tile * CM_TILE;
        const int npx = P - p0 < CM_TILE ? (int)(P - p0) : CM_TILE;
        const uint8_t* gls = labels + (long long)s * P + p0;
        const uint8_t* gln = labels + (long long)n * P + p0;
        const uint8_t* gis = images + ((long long)s * P + p0) * 3;
        const uint8_t* gin = images + ((long long)n * P + p0) * 3;
        uint8_t* glo = out_labels + (long long)n * P + p0;
        uint8_t* gio = out_images + ((long long)n * P + p0) * 3;
        cm_put(r.ls, ls, t, CM_LSTRIP / 16);
        cm_put(r.ln, ln, CM_THREADS - 1 - t, CM_LSTRIP / 16);
        cm_put(r.is, is, t, CM_ISTRIP / 16);
        cm_put(r.in, in, t, CM_ISTRIP / 16);
        __syncthreads();                                                                        // the four strips (and, in the first trip, the table) are filled
        if (tile + gridDim.x < tiles) r = cm_fetch_tile(images, labels, s, n, N, P, tile + gridDim.x, t);   // in flight while this tile is mixed and stored
        const int s_ls = (int)((uintptr_t)gls & 15), s_ln = (int)((uintptr_t)gln & 15), s_lo = (int)((uintptr_t)glo & 15);
        const int s_is = (int)((uintptr_t)gis & 15), s_in = (int)((uintptr_t)gin & 15), s_io = (int)((uintptr_t)gio & 15);
        if (((s_ls | s_ln | s_lo | s_is | s_in | s_io) & 3) == 0) {
            // dwords.  Pixels from npx on give bytes behind the tile's end in lo / io, which are not stored.
            const unsigned int a = *reinterpret_cast<const unsigned int*>(ls + s_ls + 4 * t);
            const unsigned int b = *reinterpret_cast<const unsigned int*>(ln + s_ln + 4 * t);
            const unsigned int f0 = tab[a & 255u] ? 0xFFu : 0u, f1 = tab[(a >> 8) & 255u] ? 0xFFu : 0u;
            const unsigned int f2 = tab[(a >> 16) & 255u] ? 0xFFu : 0u, f3 = tab[a >> 24] ? 0xFFu : 0u;
            const unsigned int ml = f0 | (f1 << 8) | (f2 << 16) | (f3 << 24);
            *reinterpret_cast<unsigned int*>(lo + s_lo + 4 * t) = (a & ml) | (b & ~ml);
            // the 12 bytes of four pixels: p0 p0 p0 p1 | p1 p1 p2 p2 | p2 p3 p3 p3 (lowest byte first)
            const unsigned int m[3] = {f0 * 0x00010101u | (f1 << 24), f1 * 0x00000101u | f2 * 0x01010000u, f2 | f3 * 0x01010100u};
            const unsigned int* xs = reinterpret_cast<const unsigned int*>(is + s_is + 12 * t);
            const unsigned int* xn = reinterpret_cast<const unsigned int*>(in + s_in + 12 * t);
            unsigned int* xo = reinterpret_cast<unsigned int*>(io + s_io + 12 * t);
#pragma unroll
            for (int j = 0; j < 3; ++j) xo[j] = (xs[j] & m[j]) | (xn[j] & ~m[j]);
        } else {
            for (int q = 4 * t; q < 4 * t + 4 && q < npx; ++q) {
                const uint8_t c = ls[s_ls + q];
                const bool take = tab[c] != 0;
                lo[s_lo + q] = take ? c : ln[s_ln + q];
                const uint8_t* x = take ? is + s_is + 3 * q : in + s_in + 3 * q;
                for (int j = 0; j < 3; ++j) io[s_io + 3 * q + j] = x[j];
            }
        }
        __syncthreads();                                                                        // the input strips are free for the next tile; lo and io are whole
        cm_store_lines(glo, npx, lo, t);
        cm_store_lines(gio, 3 * npx, io, t);
    }
}

void launch_class_mix(const uint8_t* images, const uint8_t* labels, const int* src, int N, long long P, int C, unsigned long long seed,
                      unsigned long long draw, void* work, uint8_t* out_images, uint8_t* out_labels, uint8_t* selected_out, hipStream_t s)
{
    const CmWork w = cm_work(work, N);
    const int words = N * 8;
    hipLaunchKernelGGL(class_mix_clear_kernel, dim3((words + CM_THREADS - 1) / CM_THREADS), dim3(CM_THREADS), 0, s, w.presence, w.flag, words);
    const long long per_image = (CM_BLOCKS + N - 1) / N;
    const long long lines = (P + 15) / 16, pblocks = (lines + CM_THREADS * CM_PRESENCE_LOADS - 1) / (CM_THREADS * CM_PRESENCE_LOADS);
    hipLaunchKernelGGL(class_mix_presence_kernel, dim3((unsigned)(pblocks < per_image ? pblocks : per_image), N), dim3(CM_THREADS), 0, s, labels, P,
                       (unsigned int)C, w.presence);
    hipLaunchKernelGGL(class_mix_select_kernel, dim3(N), dim3(CM_THREADS), 0, s, src, N, C, seed, draw, w, selected_out);
    const long long tiles = (P + CM_TILE - 1) / CM_TILE;
    hipLaunchKernelGGL(class_mix_kernel, dim3((unsigned)(tiles < per_image ? tiles : per_image), N), dim3(CM_THREADS), 0, s, images, labels, src, N, P,
                       w.table, out_images, out_labels);
}

}  // namespace fcn8s
