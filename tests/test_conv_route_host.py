"""csrc/conv_route.h, the rules that decide which kernels a convolution layer runs through, is host-only C++: a stand-alone program (below) includes
it, is built by the host compiler with AddressSanitizer + UBSan and asserts (a) the Winograd tile the cost rule picks on maps worked out by hand,
and (b), exhaustively over widths / options / maps, the implications between the rules that the launch sequences of model.hip rely on: whoever is
promised a buffer takes the path that reads it, and every route fits the scratch the plan sizes."""
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
#define IMPLIES(a, b) do { if ((a) && !(b)) { std::fprintf(stderr, "line %d: %s  =/=>  %s   [cin %d cout %d nb %d min_cin %d tile %d N %d map %dx%d]\n", \
    __LINE__, #a, #b, cin, cout, nb, o.wino_min_cin, o.wino_tile, N, H, W); std::exit(1); } } while (0)

static RouteOpts opts(int N = 2) { RouteOpts o; o.plan_N = N; o.scratch = true; return o; }
// floats of a [P][T][C] tensor of F(tile x tile, 3x3): winograd.hip's wino_alpha (tile + 2), wino_tiles and wino_slab (T * C + 1088), restated
static long long wino_floats(int tile, int N, int H, int W, int C)
{
    const long long T = (long long)N * ((H + tile - 1) / tile) * ((W + tile - 1) / tile);
    return (long long)(tile + 2) * (tile + 2) * (T * C + 1088);
}

int main()
{
    {   // (a) tiles, each derivable by hand from the cost rule (multiplies per channel pair: 64 per F(6x6) tile, 36 per F(4x4) tile, 16 per F(2x2) tile)
        CHECK(wino_tile_for(opts(1), 32, 64) == 4);            // one image: 66 F(6x6) tiles round up to 128 GEMM rows, 64 * 128 > 36 * 128
        CHECK(wino_tile_for(opts(2), 32, 64) == 6);            // a batch: 64 * 66 < 36 * 128
        CHECK(wino_tile_for(opts(16), 512, 1024) == 6);        // 64 * 86 * 171 < 36 * 128 * 256
        CHECK(wino_tile_for(opts(2), 6, 6) == 6);              // 64 * 1 < 16 * 9 (6 % 4 != 0: F(2x2) is the alternative)
        for (int K : {3, 7}) { CHECK(wino_tile_for(opts(), 31, 64, K) == 0); CHECK(wino_tile_for(opts(), 32, 63, K) == 0); CHECK(wino_tile_for(opts(1), 33, 65, K) == 0); }
        { RouteOpts o = opts(); o.wino_tile = 4; CHECK(wino_tile_for(o, 30, 30) == 2); }
        { RouteOpts o = opts(); o.wino_force_tile = 4; CHECK(wino_tile_for(o, 30, 30) == 0); }
        { RouteOpts o = opts(); o.wino_force_tile = 6; CHECK(wino_tile_for(o, 30, 30) == 6); }
        CHECK(wino_tile_for(opts(), 16, 32, 7) == 4);
        CHECK(wino_tile_for(opts(), 10, 14, 7) == 0);
        { RouteOpts o = opts(); o.wino_tile_hires = 4; o.wino_hires_pixels = 100000;
          CHECK(wino_tile_for(o, 512, 1024) == 4);             // 524288 pixels: capped
          CHECK(wino_tile_for(o, 128, 256) == 6); }            // 32768 pixels: not capped; 64 * 22 * 43 < 36 * 32 * 64
    }
    // (b) the implications.  The three layers of the sweep: L (cin -> cout), its in-block successor X (cout -> cout: a block has one width), and
    // a successor of another width X2 (cout -> nb) where a rule takes any two adjacent layers.
    const int widths[] = {4, 16, 32, 64, 128, 192, 256, 512};
    const int maps[][2] = {{32, 32}, {32, 64}, {48, 80}, {96, 160}, {192, 192}, {512, 1024}};
    long long swept = 0, routed = 0;
    for (int cin : widths) for (int cout : widths) for (int nb : widths)
    for (int min_cin : {0, 16, 64, 128}) for (int tile : {2, 4, 6}) for (int N : {1, 2}) for (const auto& hw : maps) {
        const int H = hw[0], W = hw[1];
        RouteOpts o = opts(N); o.wino_min_cin = min_cin; o.wino_tile = tile;
        const ConvShape L{N, H, W, cin, cout, 3}, X{N, H, W, cout, cout, 3}, X2{N, H, W, cout, nb, 3};
        ++swept;
        // dM promised to L by X's data gradient (the promise is made inside X's adjoint path): L's weight gradient takes the prefilled adjoint
        // branch -- it runs in the Winograd domain (keeps V) and asks adjoint_dgrad(L).  broken_promise is unreachable by rule.
        IMPLIES(dm_from_next(o, L) && adjoint_dgrad(o, X), keeps_v(o, L) && adjoint_dgrad(o, L));
        // a pool routed in the transform: the last conv keeps V and its data gradient's input transform is fused (has_prev: cin == cout)
        for (bool has_prev : {false, true}) {
            if (has_prev && cin != cout) continue;
            IMPLIES(pool_in_transform(o, L, has_prev), keeps_v(o, L) && dgrad_input_fused(o, L));
            IMPLIES(pool_in_transform(o, L, has_prev), has_prev);
        }
        // an output transform fused into the next layer's input transform: both run F(6x6) (one tile grid: the same map), and the next keeps V
        for (const ConvShape& nx : {X, X2}) {
            IMPLIES(out_in_fused(o, L, nx), fwd_tile(o, L) == 6 && fwd_tile(o, nx) == 6 && wino_tile_for(o, L.H, L.W) == wino_tile_for(o, nx.H, nx.W));
            IMPLIES(out_in_fused(o, L, nx), keeps_v(o, nx));
        }
        // a ReLU bit record exists: its writer's route is Winograd
        for (bool conv1_1 : {false, true}) {
            if (conv1_1 && cin != 4) continue;
            const RbWriter wr = relu_record_writer(o, L, X, conv1_1);
            IMPLIES(wr == RbWriter::self, fwd_tile(o, L) != 0);
            IMPLIES(wr == RbWriter::consumer, fwd_tile(o, X) != 0 && conv1_1);
        }
        // conv1_1 inside conv1_2's input transform: conv1_2 runs F(6x6) and keeps V, and the record the backward pass masks with has a writer
        if (cin == 4) {
            IMPLIES(conv1_in_next_transform(o, L, X), fwd_tile(o, X) == 6 && keeps_v(o, X));
            IMPLIES(conv1_in_next_transform(o, L, X), relu_record_writer(o, L, X, true) == RbWriter::consumer);
        }
        // the fusions of the backward pass sit on a Winograd data gradient, the adjoint one on a fused-input one
        IMPLIES(adjoint_dgrad(o, L), dgrad_input_fused(o, L));
        IMPLIES(dgrad_input_fused(o, L), dgrad_tile(o, L) >= 4);
        // every Winograd route's V and M fit the scratch the plan rule sizes on this map (V, M: Cin / Cout channels forward, swapped backward)
        if (fwd_tile(o, L) || dgrad_tile(o, L) || keeps_v(o, L)) {
            ++routed;
            const int t = wino_tile_for(o, H, W), c = scratch_channels(o, L);
            IMPLIES(true, t != 0 && c != 0);
            IMPLIES(true, wino_floats(t, N, H, W, cin) <= wino_floats(t, N, H, W, c) && wino_floats(t, N, H, W, cout) <= wino_floats(t, N, H, W, c));
            IMPLIES(fwd_tile(o, L) != 0, fwd_tile(o, L) == t);
            IMPLIES(dgrad_tile(o, L) != 0, dgrad_tile(o, L) == t);
        }
        // without the scratch nothing that needs it runs
        RouteOpts n = o; n.scratch = false;
        CHECK(!fwd_tile(n, L) && !dgrad_tile(n, L) && !dgrad_input_fused(n, L) && !adjoint_dgrad(n, L) && !out_in_fused(n, L, X) &&
              !conv1_in_next_transform(n, L, X) && !dm_from_next(n, L) && !pool_in_transform(n, L, true));
        // winograd_min_cin = 0: no 3x3 route at all
        if (min_cin == 0) CHECK(!fwd_tile(o, L) && !keeps_v(o, L) && !dgrad_tile(o, L) && !scratch_channels(o, L) && relu_record_writer(o, L, X, cin == 4) == RbWriter::none);
    }
    CHECK(swept == 8LL * 8 * 8 * 4 * 3 * 2 * 6 && routed > swept / 10);      // (the sweep did reach Winograd routes)
    CHECK(bt_gemm_ok(64, 64) && bt_gemm_ok(512, 512) && bt_gemm_ok(4096, 2048) && !bt_gemm_ok(64, 192) && !bt_gemm_ok(8, 64));
    std::puts("conv_route ok");
    return 0;
}
"""


def test_conv_route_rules_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "conv_route_main.cc"
    exe = tmp_path / "conv_route_main"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "fcn8s_tensorflow_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "conv_route ok", r.stdout + r.stderr
