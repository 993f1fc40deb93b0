"""The bf16_train section of csrc/conv_route.h -- which fp32 tensor a pass of that precision keeps and which it skips -- is host-only C++ like the
rest of the header: a stand-alone program (below) includes it, is built by the host compiler with AddressSanitizer + UBSan and asserts, exhaustively
over the mode's widths (multiples of 64) / blocks / positions / options / maps, the promise the launch sequences of model.hip rely on: the forward
pass skips an fp32 tensor only if every later reader takes the bf16 form (the deferred errors of conv_wgrad / conv_dgrad are unreachable by rule)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "conv_route.h"
#include <cstdio>
#include <cstdlib>
using namespace fcn8s;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
// an implication over the sweep: says where it broke
#define IMPLIES(a, b) do { if ((a) && !(b)) { std::fprintf(stderr, "line %d: %s  =/=>  %s   [block %d pos %d widths %d %d %d acts %d fuse_pool %d conv1_tiled %d copies %d N %d map %dx%d]\n", \
    __LINE__, #a, #b, blk, pos, wp, wb, wn, o.acts, o.fuse_pool, o.conv1_tiled, o.copies, N, H, W); std::exit(1); } } while (0)
// both sides of a rule were reached
struct Seen { long long yes = 0, no = 0; bool operator()(bool v) { ++(v ? yes : no); return v; } };

int main()
{
    // by hand
    CHECK(bf16_kernels_take(ConvShape{2, 32, 32, 64, 64, 3}) && bf16_kernels_take(ConvShape{1, 4, 4, 512, 4096, 7}) && bf16_kernels_take(ConvShape{1, 4, 4, 4096, 4096, 1}));
    CHECK(!bf16_kernels_take(ConvShape{2, 32, 32, 4, 64, 3}) && !bf16_kernels_take(ConvShape{2, 32, 32, 64, 96, 3}) && !bf16_kernels_take(ConvShape{2, 32, 32, 32, 64, 3}) &&
          !bf16_kernels_take(ConvShape{2, 32, 32, 64, 64, 2}));
    CHECK(!pool_feeds_skip(1) && !pool_feeds_skip(2) && pool_feeds_skip(3) && pool_feeds_skip(4) && !pool_feeds_skip(5));
    CHECK(bf16_plane_fits(0) && bf16_plane_fits(32LL * 16 * 1026 * 514) && !bf16_plane_fits(32LL * 128 * 1026 * 514) && !bf16_plane_fits(1LL << 31));
    {   // conv1_1's bf16-only form wants whole 8 x 16 tiles and the 64-column tile
        const Bf16Opts o;
        CHECK(conv1_writes_bf16_only(o, ConvShape{1, 32, 32, 4, 64, 3}, ConvShape{1, 32, 32, 64, 64, 3}));
        CHECK(!conv1_writes_bf16_only(o, ConvShape{1, 36, 32, 4, 64, 3}, ConvShape{1, 36, 32, 64, 64, 3}));
        CHECK(!conv1_writes_bf16_only(o, ConvShape{1, 32, 40, 4, 64, 3}, ConvShape{1, 32, 40, 64, 64, 3}));
        CHECK(!conv1_writes_bf16_only(o, ConvShape{1, 32, 32, 4, 32, 3}, ConvShape{1, 32, 32, 32, 64, 3}));
    }
    // The sweep: block blk (width wb, 2 / 2 / 3 / 3 / 3 convs) between a block of width wp and a consumer of width wn (the next block's first conv, or
    // fc6 with K = 7 behind block 5); layer l at position pos, its in-block successor X, the block's last conv `last` and the pool's consumer `cons`.
    const int widths[] = {64, 128, 192, 256, 512, 4096};
    const int nconv[] = {2, 2, 3, 3, 3};
    const int maps[][2] = {{32, 32}, {32, 64}, {48, 80}, {96, 160}, {192, 192}, {512, 1024}};
    long long swept = 0;
    Seen s_conv1, s_copy, s_only, s_poolin, s_routes, s_pout, s_pout_only, s_preads, s_fc7, s_dy, s_pbwd;
    for (int wp : widths) for (int wb : widths) for (int wn : widths) for (int blk = 1; blk <= 5; ++blk) for (int pos = 1; pos <= nconv[blk - 1]; ++pos)
    for (int bits = 0; bits < 16; ++bits) for (int N : {1, 2}) for (const auto& hw : maps) {
        const int H = hw[0], W = hw[1];
        Bf16Opts o; o.acts = bits & 1; o.fuse_pool = bits & 2; o.conv1_tiled = bits & 4; o.copies = bits & 8;
        const bool conv1_1 = blk == 1 && pos == 1, has_next = pos < nconv[blk - 1];
        const ConvShape l{N, H, W, pos > 1 ? wb : (blk == 1 ? 4 : wp), wb, 3}, X{N, H, W, wb, wb, 3}, last = X;
        const ConvShape cons{N, H / 2, W / 2, wb, wn, blk == 5 ? 7 : 3};
        ++swept;
        // the sweep's construction: a block's last conv has a conv of the block's width in front of it, and conv1_1 alone has Cin % 64 != 0
        CHECK(nconv[blk - 1] >= 2 && last.Cin == last.Cout);
        CHECK(conv1_1 == (l.Cin % 64 != 0));
        // 1. a conv output kept only as bf16 (recorded as in_bf16_only(consumer)): the consumer (X, never conv1_1: its position is pos + 1 >= 2)
        //    finds its input in the weight gradient and its mask in the data gradient on the bf16 kernels
        if (has_next) {
            const bool only = conv1_1 ? s_conv1(conv1_writes_bf16_only(o, l, X)) : s_only(out_bf16_only(o, l, X));
            IMPLIES(only, bf16_kernels_take(X) && bf16_kernels_take(transposed(X)));
            IMPLIES(only, pos + 1 >= 2 && X.Cin % 64 == 0);
            IMPLIES(only && !conv1_1, out_bf16_copy(o, has_next));          // (the copy it is the only form of is written)
            IMPLIES(conv1_1, !out_bf16_only(o, l, X));                      // (conv1_1 has its own rule: the generic one refuses 4 input channels)
        }
        s_copy(out_bf16_copy(o, has_next));
        if (!has_next) {
            // 2. the last conv wrote only the pool's bf16 input: the pool never looks for the fp32 tensor
            const bool pin = s_poolin(pool_in_bf16(o, last, cons, blk));
            IMPLIES(pin, pool_routes(o, last) && pool_out_bf16_only(o, last, cons, blk) && pool_reads_bf16(o, last, cons, blk));
            IMPLIES(pin, !pool_feeds_skip(blk));
            // 3. a pool output kept only as bf16 (in_bf16_only(cons)): no skip head reads it, and its consumer -- the next block's first conv or
            //    fc6, never conv1_1 -- takes the bf16 kernels in both gradients
            const bool pout_only = s_pout_only(pool_out_bf16_only(o, last, cons, blk));
            IMPLIES(pout_only, !pool_feeds_skip(blk));
            IMPLIES(pout_only, bf16_kernels_take(cons) && bf16_kernels_take(transposed(cons)) && cons.Cin % 64 == 0);
            IMPLIES(pout_only, pool_out_bf16(o, last, cons) && pool_routes(o, last));
            IMPLIES(s_preads(pool_reads_bf16(o, last, cons, blk)), pout_only);      // (the bf16-input pool kernel has no fp32 output)
            const bool routes = s_routes(pool_routes(o, last));
            IMPLIES(s_pout(pool_out_bf16(o, last, cons)), routes);
            // 5. the pool's backward kernel writes no fp32 dZ: the last conv's weight gradient (and data gradient) take the copy
            IMPLIES(s_pbwd(pool_bwd_writes_bf16(o, last)), bf16_kernels_take(last) && bf16_kernels_take(transposed(last)));
        }
        // 4. l's output gradient exists only as a bf16 copy (written by X's data gradient): never conv1_1, both of l's gradients fit
        if (has_next) {
            const bool dy = s_dy(dy_bf16_only(o, l, conv1_1, X));
            IMPLIES(dy, !conv1_1);
            IMPLIES(dy, bf16_kernels_take(l) && bf16_kernels_take(transposed(l)));
            IMPLIES(dy, bf16_kernels_take(transposed(X)));                  // (the launch that writes the copy is a bf16 one)
        }
        s_fc7(fc7_in_from_fc6(o));
        // 6. bf16_acts = 0: nothing is kept "only" as bf16.  No copies (an evaluation pass with bf16_infer_copies = 0): no forward rule makes one
        if (!o.acts)
            CHECK(!conv1_writes_bf16_only(o, l, X) && !out_bf16_only(o, l, X) && !pool_in_bf16(o, last, cons, blk) && !pool_out_bf16_only(o, last, cons, blk) &&
                  !pool_reads_bf16(o, last, cons, blk) && !dy_bf16_only(o, l, conv1_1, X));
        if (!o.copies)
            CHECK(!conv1_writes_bf16_only(o, l, X) && !out_bf16_copy(o, true) && !out_bf16_only(o, l, X) && !pool_in_bf16(o, last, cons, blk) && !pool_routes(o, last) &&
                  !pool_out_bf16(o, last, cons) && !pool_out_bf16_only(o, last, cons, blk) && !pool_reads_bf16(o, last, cons, blk) && !fc7_in_from_fc6(o));
    }
    CHECK(swept == 6LL * 6 * 6 * 13 * 16 * 2 * 6);
    // the sweep reached both sides of every rule
    for (const Seen* s : {&s_conv1, &s_copy, &s_only, &s_poolin, &s_routes, &s_pout, &s_pout_only, &s_preads, &s_fc7, &s_dy, &s_pbwd})
        CHECK(s->yes > swept / 1000 && s->no > swept / 1000);
    std::puts("bf16_route ok");
    return 0;
}
"""


def test_bf16_train_rules_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "bf16_route_main.cc"
    exe = tmp_path / "bf16_route_main"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "fcn8s_tensorflow_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bf16_route ok", r.stdout + r.stderr
