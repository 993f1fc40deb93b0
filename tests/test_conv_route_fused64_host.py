"""csrc/conv_route.h, rule gemm_out_fused64 -- conv1_2, the last conv of block 1, runs its position GEMMs, output transform and pool in one kernel
(wino_gemm_out64_kernel) -- checked by a stand-alone host program, built like tests/test_conv_route_host.py's: what the launch sequence of
model.hip relies on (F(6x6), both widths 64, the pool routed in the transform), that the rule never reads the batch, and that the options which
switch the Winograd route or F(6x6) off switch it off too."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "conv_route.h"
#include <cstdio>
#include <cstdlib>
using namespace fcn8s;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s   [cin %d cout %d min_cin %d tile %d plan_N %d map %dx%d]\n", \
    __LINE__, #c, cin, cout, o.wino_min_cin, o.wino_tile, o.plan_N, H, W); std::exit(1); } } while (0)

int main()
{
    const int widths[] = {4, 16, 32, 64, 128, 192};
    const int maps[][2] = {{12, 12}, {32, 32}, {32, 64}, {64, 64}, {48, 80}, {96, 160}, {512, 1024}, {1024, 2048}};
    long long swept = 0, taken = 0;
    for (int cin : widths) for (int cout : widths) for (int min_cin : {0, 16, 64, 128}) for (int tile : {2, 4, 6}) for (int plan_N : {1, 2, 3, 16})
    for (const auto& hw : maps) for (bool has_prev : {false, true}) for (bool scratch : {false, true}) {
        const int H = hw[0], W = hw[1];
        RouteOpts o; o.plan_N = plan_N; o.scratch = scratch; o.wino_min_cin = min_cin; o.wino_tile = tile;
        const ConvShape L{plan_N, H, W, cin, cout, 3};
        const bool f = gemm_out_fused64(o, L, has_prev, true);
        ++swept; taken += f;
        // what conv_winograd's launch relies on
        if (f) CHECK(fwd_tile(o, L) == 6 && L.Cin == 64 && L.Cout == 64 && pool_in_transform(o, L, has_prev) && keeps_v(o, L) && has_prev && scratch);
        // the rule reads the shape, never the batch: the same answer for every N ...
        for (int N : {1, 2, 5, 16, 1000}) { ConvShape M = L; M.N = N; CHECK(gemm_out_fused64(o, M, has_prev, true) == f); }
        // ... and for every plan_N, except through the tile itself: wino_tile_for treats a single image's small map apart (plan_N == 1 rounds the
        // GEMM rows up), and where that changes the tile the whole algorithm changes.  Among batches of two or more nothing may differ; between
        // one image and a batch only where the tile does.
        for (int pn : {1, 2, 3, 7, 16, 64}) {
            RouteOpts p = o; p.plan_N = pn;
            if ((pn == 1) == (plan_N == 1) || wino_tile_for(p, H, W) == wino_tile_for(o, H, W)) CHECK(gemm_out_fused64(p, L, has_prev, true) == f);
        }
        // off wherever the Winograd route or F(6x6) is off
        if (min_cin == 0 || tile == 4 || tile == 2) CHECK(!f);
        { RouteOpts p = o; p.wino_min_cin = 0; CHECK(!gemm_out_fused64(p, L, has_prev, true)); }
        { RouteOpts p = o; p.wino_tile = 4; CHECK(!gemm_out_fused64(p, L, has_prev, true)); }
        // only conv1_2: the same shape as the last conv of a deeper block keeps the two kernels
        CHECK(!gemm_out_fused64(o, L, has_prev, false));
        // a 7x7 layer never
        { ConvShape M = L; M.K = 7; CHECK(!gemm_out_fused64(o, M, has_prev, true)); }
    }
    {   // the shapes it exists for, by hand: conv1_2 at the training shape, at one full-size image, and on the small maps of the GPU test
        int cin = 64, cout = 64, H = 0, W = 0; RouteOpts o; o.scratch = true;
        o.plan_N = 16; CHECK(gemm_out_fused64(o, ConvShape{16, 512, 1024, 64, 64, 3}, true, true));
        o.plan_N = 1;  CHECK(gemm_out_fused64(o, ConvShape{1, 512, 1024, 64, 64, 3}, true, true));
        o.plan_N = 4;  CHECK(gemm_out_fused64(o, ConvShape{4, 1024, 2048, 64, 64, 3}, true, true));
        o.plan_N = 1;  CHECK(gemm_out_fused64(o, ConvShape{1, 64, 64, 64, 64, 3}, true, true));             // 121 tiles: 64 * 128 < 36 * 256
        o.plan_N = 2;  CHECK(gemm_out_fused64(o, ConvShape{2, 32, 64, 64, 64, 3}, true, true));             // 132 tiles: 64 * 66 < 36 * 128
        o.plan_N = 1;  CHECK(!gemm_out_fused64(o, ConvShape{1, 32, 64, 64, 64, 3}, true, true));            // one image: F(4x4) (tests/test_conv_route_host.py)
        o.plan_N = 16; CHECK(!gemm_out_fused64(o, ConvShape{16, 256, 512, 128, 128, 3}, true, true));       // conv2_2: 128 wide
        (void)cin; (void)cout; (void)H; (void)W;
    }
    if (!(taken > 0 && taken < swept / 20)) { std::fprintf(stderr, "the sweep took the route %lld times of %lld\n", taken, swept); return 1; }
    std::puts("conv_route fused64 ok");
    return 0;
}
"""


def test_gemm_out_fused64_rule_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "conv_route_fused64_main.cc"
    exe = tmp_path / "conv_route_fused64_main"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "fcn8s_tensorflow_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "conv_route fused64 ok", r.stdout + r.stderr
