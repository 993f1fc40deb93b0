"""csrc/split_route.h, the rules that decide into how many K slabs a launch cuts its dot products, is host-only C++: a stand-alone program (below)
includes it, is built by the host compiler with AddressSanitizer + UBSan and holds every rule to its contract against a transcription
(`parent_*`) of the formulas launch_conv_bf16_256 and launch_head_fwd_c had inline before the rules existed:

  (1) for N >= 2 the answer does not depend on N;
  (2) for N == 1 it may differ (SINGLE_IMAGE_EXCEPTIONS of tests/test_batch_independence_ops_gpu.py names the tested cases);
  (3) for N == 1 it is the inline formula's: batch-1 inference keeps its kernels;
  (4) at the benchmark legs' shapes (fp32 16 x 1024x512, bf16_train 4 x 2048x1024, every 3x3 / fc6 / fc7 / score layer of the default widths)
      it is the inline formula's too: no benchmark leg changes kernels;
  (5) the threshold cases of tests/test_batch_independence_ops_gpu.py do straddle the inline formulas' thresholds -- the slab counts written in
      that file's comments, recomputed here -- so those GPU cases fail on the inline formulas and mean something."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fcn8s_tensorflow_amd", "csrc")

PROGRAM = r"""
#include "split_route.h"
#include <cstdio>
#include <cstdlib>
using namespace fcn8s;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
#define SAME(a, b) do { const long long a_ = (a), b_ = (b); if (a_ != b_) { std::fprintf(stderr, "line %d: %s = %lld, %s = %lld   [N %d map %dx%d cin %d cout %d K %d]\n", \
    __LINE__, #a, a_, #b, b_, s.N, s.H, s.W, s.Cin, s.Cout, s.K); std::exit(1); } } while (0)

// ---- the formulas as the launchers had them inline (gemm_bf16.hip: G_BM = 256 rows, G_BK = 32 channels; skinny.hip: 32-row blocks, 8 slabs) ----
static int parent_rows(const ConvShape& s, int tbn, int tbm)           // conv_bf16_rows_kernel: blocks over ALL N (H + 2)(W + 2) padded positions
{
    const long long R = (long long)s.N * (s.H + 2) * (s.W + 2);
    const unsigned blocks = (unsigned)(((R + tbm - 1) / tbm) * (s.Cout / tbn));
    const long long nkt_all = 3LL * (s.Cin / 32);
    if (tbn == 64 && blocks <= 48 && nkt_all >= 24) {
        long long ks = 256 / blocks; if (ks > 8) ks = 8; if (ks > nkt_all / 6) ks = nkt_all / 6;
        if (ks >= 2) return (int)ks;
    }
    return 1;
}
static int parent_gemm_fwd(const ConvShape& s)                         // conv_bf16_256_kernel<256>, forward epilogue, K != 3
{
    const long long M = (long long)s.N * s.H * s.W, rt0 = (M + 255) / 256, nkt_all = (long long)s.K * s.K * s.Cin / 32;
    if (s.Cout % 256 == 0 && rt0 * (s.Cout / 256) <= 64 && nkt_all >= 64) {
        long long ks = 256 / (rt0 * (s.Cout / 256));
        if (ks > 8) ks = 8;
        if (ks > nkt_all / 16) ks = nkt_all / 16;
        if (ks >= 2) return (int)ks;
    }
    return 1;
}
static int parent_head(const ConvShape& s)                             // head_fwd_kernel: K = s.Cin channels, C = s.Cout classes
{
    const long long M = (long long)s.N * s.H * s.W;
    const unsigned blocks = (unsigned)((M + 31) / 32);
    return (blocks <= 64 && s.Cin % (8 * 16 * 32) == 0 && (M * s.Cout) % 4 == 0) ? 8 : 1;
}

static const int kNs[] = {1, 2, 3, 5, 16, 64, 1000};

int main()
{
    long long swept = 0, split1 = 0, differs = 0;
    const int maps[][2] = {{2, 2}, {5, 7}, {6, 10}, {8, 8}, {12, 20}, {16, 16}, {16, 32}, {32, 16}, {30, 34}, {32, 64}, {64, 32}, {64, 128}, {128, 64}, {256, 512}, {512, 1024}, {1024, 2048}};
    const int chans[] = {64, 128, 192, 256, 384, 512, 1024, 2048, 4096};
    // (1), (3) over the sweep
    for (const auto& hw : maps) for (int cin : chans) for (int cout : chans) {
        int at2[8] = {0};
        for (int N : kNs) {
            // rows kernel, both forms
            int f = 0;
            for (int form : {64, 128}) {
                if (form == 128 && cout % 128) { ++f; continue; }
                const ConvShape s{N, hw[0], hw[1], cin, cout, 3};
                const int tbm = form == 64 ? 256 : 128;
                const int got = bf16_rows_slabs(s, form, tbm);
                ++swept;
                CHECK(got >= 1 && got <= 8);
                if (N == 1) { SAME(got, parent_rows(s, form, tbm)); split1 += got > 1; }
                else if (N == 2) { at2[f] = got; differs += got != bf16_rows_slabs(ConvShape{1, hw[0], hw[1], cin, cout, 3}, form, tbm); }
                else SAME(got, at2[f]);
                ++f;
            }
            for (int K : {1, 7}) {
                const ConvShape s{N, hw[0], hw[1], cin, cout, K};
                const int got = bf16_gemm_fwd_slabs(s);
                ++swept;
                CHECK(got >= 1 && got <= 8);
                if (N == 1) { SAME(got, parent_gemm_fwd(s)); split1 += got > 1; }
                else if (N == 2) { at2[f] = got; differs += got != bf16_gemm_fwd_slabs(ConvShape{1, hw[0], hw[1], cin, cout, K}); }
                else SAME(got, at2[f]);
                ++f;
            }
            for (int classes : {20, 4}) {
                const ConvShape s{N, hw[0], hw[1], cin, classes, 1};
                const int got = head_fwd_splits(s);
                ++swept;
                CHECK(got == 1 || got == kHeadSplits);
                if (N == 1) { SAME(got, parent_head(s)); split1 += got > 1; }
                else if (N == 2) { at2[f] = got; differs += got != head_fwd_splits(ConvShape{1, hw[0], hw[1], cin, classes, 1}); }
                else SAME(got, at2[f]);
                ++f;
            }
        }
    }
    CHECK(swept == 16LL * 9 * 9 * 7 * 6 - 16LL * 9 * 2 * 7 && split1 > 100 && differs == split1);     // (the sweep did reach splits; N = 2 differs from N = 1 exactly where N = 1 splits)
    // (4) the benchmark legs: fp32 16 x 1024x512 and bf16_train 4 x 2048x1024, default widths 64, 128, 256, 512, 512, 4096, 4096
    struct Leg { int N, H, W; };
    for (const Leg leg : {Leg{16, 512, 1024}, Leg{4, 1024, 2048}}) {
        struct L3 { int shift, cin, cout; };
        const L3 l3[] = {{0, 64, 64}, {1, 64, 128}, {1, 128, 128}, {2, 128, 256}, {2, 256, 256}, {3, 256, 512}, {3, 512, 512}, {4, 512, 512}};
        for (const L3& l : l3) for (int form : {64, 128}) for (bool bwd : {false, true}) {
            if (form == 128 && (bwd ? l.cin : l.cout) % 128) continue;
            const ConvShape s{leg.N, leg.H >> l.shift, leg.W >> l.shift, bwd ? l.cout : l.cin, bwd ? l.cin : l.cout, 3};
            SAME(bf16_rows_slabs(s, form, form == 64 ? 256 : 128), parent_rows(s, form, form == 64 ? 256 : 128));
        }
        { const ConvShape s{leg.N, leg.H >> 5, leg.W >> 5, 512, 4096, 7}; SAME(bf16_gemm_fwd_slabs(s), parent_gemm_fwd(s)); }
        { const ConvShape s{leg.N, leg.H >> 5, leg.W >> 5, 4096, 4096, 1}; SAME(bf16_gemm_fwd_slabs(s), parent_gemm_fwd(s)); }
        { const ConvShape s{leg.N, leg.H >> 5, leg.W >> 5, 4096, 20, 1}; SAME(head_fwd_splits(s), parent_head(s)); }
        { const ConvShape s{leg.N, leg.H >> 4, leg.W >> 4, 512, 20, 1}; SAME(head_fwd_splits(s), parent_head(s)); }
        { const ConvShape s{leg.N, leg.H >> 3, leg.W >> 3, 256, 20, 1}; SAME(head_fwd_splits(s), parent_head(s)); }
    }
    // (5) the threshold cases of the GPU file: what the inline formulas gave at each tested N, and what the rules give
    auto rows = [](int N) { return ConvShape{N, 16, 16, 512, 512, 3}; };
    CHECK(parent_rows(rows(1), 64, 256) == 8 && parent_rows(rows(2), 64, 256) == 8 && parent_rows(rows(4), 64, 256) == 5 && parent_rows(rows(5), 64, 256) == 1);
    CHECK(bf16_rows_slabs(rows(1), 64, 256) == 8 && bf16_rows_slabs(rows(2), 64, 256) == 1 && bf16_rows_slabs(rows(4), 64, 256) == 1 && bf16_rows_slabs(rows(5), 64, 256) == 1);
    auto fc7 = [](int N) { return ConvShape{N, 16, 16, 2048, 4096, 1}; };
    CHECK(parent_gemm_fwd(fc7(1)) == 4 && parent_gemm_fwd(fc7(4)) == 4 && parent_gemm_fwd(fc7(5)) == 1);
    CHECK(bf16_gemm_fwd_slabs(fc7(1)) == 4 && bf16_gemm_fwd_slabs(fc7(4)) == 1 && bf16_gemm_fwd_slabs(fc7(5)) == 1);
    auto fc7b = [](int N) { return ConvShape{N, 16, 16, 4096, 2048, 1}; };
    CHECK(parent_gemm_fwd(fc7b(1)) == 8 && parent_gemm_fwd(fc7b(2)) == 8 && parent_gemm_fwd(fc7b(5)) == 6 && parent_gemm_fwd(fc7b(8)) == 4 && parent_gemm_fwd(fc7b(9)) == 1);
    CHECK(bf16_gemm_fwd_slabs(fc7b(1)) == 8 && bf16_gemm_fwd_slabs(fc7b(2)) == 1 && bf16_gemm_fwd_slabs(fc7b(9)) == 1);
    auto fc6 = [](int N) { return ConvShape{N, 16, 16, 64, 1024, 7}; };
    CHECK(parent_gemm_fwd(fc6(1)) == 6 && parent_gemm_fwd(fc6(11)) == 5 && parent_gemm_fwd(fc6(17)) == 1);
    CHECK(bf16_gemm_fwd_slabs(fc6(1)) == 6 && bf16_gemm_fwd_slabs(fc6(11)) == 1 && bf16_gemm_fwd_slabs(fc6(17)) == 1);
    auto head = [](int N) { return ConvShape{N, 16, 32, 4096, 20, 1}; };
    CHECK(parent_head(head(1)) == 8 && parent_head(head(4)) == 8 && parent_head(head(5)) == 1);
    CHECK(head_fwd_splits(head(1)) == 8 && head_fwd_splits(head(4)) == 1 && head_fwd_splits(head(5)) == 1);
    // ... the headline image size: fc7 of one 1024x512 image (a 16x32 map) ran 8 slabs, two images 4, three or more none; a shard now computes the big batch's bits
    auto fc7h = [](int N) { return ConvShape{N, 16, 32, 4096, 4096, 1}; };
    CHECK(parent_gemm_fwd(fc7h(1)) == 8 && parent_gemm_fwd(fc7h(2)) == 4 && parent_gemm_fwd(fc7h(3)) == 1);
    CHECK(bf16_gemm_fwd_slabs(fc7h(1)) == 8 && bf16_gemm_fwd_slabs(fc7h(2)) == 1 && bf16_gemm_fwd_slabs(fc7h(3)) == 1);
    // the ragged cases of the GPU file whose single image is excepted / is not
    CHECK(head_fwd_splits(ConvShape{1, 5, 7, 4096, 20, 1}) == 8 && head_fwd_splits(ConvShape{2, 5, 7, 4096, 20, 1}) == 1 && parent_head(ConvShape{5, 5, 7, 4096, 20, 1}) == 8);
    CHECK(head_fwd_splits(ConvShape{1, 5, 7, 512, 20, 1}) == 1 && bf16_rows_slabs(ConvShape{1, 6, 10, 64, 128, 3}, 64, 256) == 1 && bf16_gemm_fwd_slabs(ConvShape{1, 6, 10, 64, 128, 7}) == 1);
    std::puts("split_route ok");
    return 0;
}
"""


def test_split_route_rules_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "split_route_main.cc"
    exe = tmp_path / "split_route_main"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "split_route ok", r.stdout + r.stderr


def test_single_image_exceptions_name_rules_that_exist():
    """SINGLE_IMAGE_EXCEPTIONS may excuse a case only by a rule that is a named function of split_route.h or conv_route.h, and only on a route
    whose launcher asks that rule (the program above evaluates the rules at those shapes: one image splits, two do not)."""
    from tests.test_batch_independence_ops_gpu import SINGLE_IMAGE_EXCEPTIONS
    text = "".join(open(os.path.join(CSRC, h)).read() for h in ("split_route.h", "conv_route.h"))
    rules = set(re.findall(r"^inline \w+ (\w+)\(", text, re.M))
    assert {"bf16_rows_slabs", "bf16_gemm_fwd_slabs", "head_fwd_splits", "wino_tile_for"} <= rules
    assert SINGLE_IMAGE_EXCEPTIONS and set(SINGLE_IMAGE_EXCEPTIONS.values()) <= rules
    kinds = {"bf16_rows_slabs": ("bf16_train_fwd/64", "bf16_train_dx/64"), "bf16_gemm_fwd_slabs": ("bf16_train_fwd/64",), "head_fwd_splits": ("conv2d/r0",)}
    for (route, shape), rule in SINGLE_IMAGE_EXCEPTIONS.items():
        assert route in kinds[rule], (route, rule)
        assert (shape[4] == 3) == (rule == "bf16_rows_slabs"), (shape, rule)
