"""csrc/pass_state.h, the model's per-pass ledger, is host-only C++: a stand-alone program (below) includes it, is built by the host compiler with
AddressSanitizer + UBSan and asserts the rules the launch sequences of model.hip rely on: a hand-off is taken exactly once and only by its own
layer, and each of the four lifetime functions clears exactly its own members."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "pass_state.h"
#include <cstdio>
#include <cstdlib>
using fcn8s::Handoff; using fcn8s::PassState;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

// every member holds something
static PassState full()
{
    PassState p;
    for (PassState::Layers* s : {&p.rbits_ok, &p.y_unwritten, &p.in_bf16_only, &p.xg16_filled, &p.q8_filled,
                                 &p.dyg16_filled, &p.db_taken, &p.dy_bf16_only, &p.dz_unwritten}) { s->insert("conv3_2"); s->insert("fc6"); }
    for (int b = 0; b < 5; ++b) p.pool_fused[b] = p.pool_routed[b] = true;
    for (Handoff* h : {&p.fft6_ready, &p.fft6_xf, &p.fwd_v, &p.dgrad_v, &p.dm, &p.dm_prefilled, &p.fft6_dyf}) h->give("fc6");
    return p;
}
static bool pools(const PassState& p, bool v) { for (int b = 0; b < 5; ++b) if (p.pool_fused[b] != v || p.pool_routed[b] != v) return false; return true; }
static bool fwd_sets(const PassState& p, size_t n) { return p.rbits_ok.size() == n && p.y_unwritten.size() == n && p.in_bf16_only.size() == n && p.xg16_filled.size() == n; }
static bool bwd_sets(const PassState& p, size_t n) { return p.db_taken.size() == n && p.dy_bf16_only.size() == n && p.dz_unwritten.size() == n; }

int main()
{
    {   // one slot, one taker
        Handoff h;
        CHECK(!h.holds("conv1_2") && !h.take("conv1_2") && !h.holds(nullptr) && !h.take(nullptr));
        h.give("conv1_2");
        CHECK(h.holds("conv1_2") && !h.holds("conv1_1") && !h.holds("conv1_22") && !h.holds("") && !h.holds(nullptr));
        CHECK(!h.take("conv2_1") && h.holds("conv1_2"));          // another layer's name: false, and the slot stays
        CHECK(h.take("conv1_2") && !h.take("conv1_2") && !h.holds("conv1_2"));      // true once, then empty
        h.give("conv3_1"); h.give("conv3_2");                     // over a full slot: replaced
        CHECK(!h.holds("conv3_1") && !h.take("conv3_1") && h.take("conv3_2"));
        h.give("fc6"); h.drop(); CHECK(!h.take("fc6"));
        h.give(nullptr); CHECK(!h.holds("") && !h.holds(nullptr));
    }
    {   // begin_forward: every forward fact and fwd_v (and the DFT slots forward() has always cleared); an fp8 pass alone clears q8_filled
        PassState p = full(); p.begin_forward(false);
        CHECK(fwd_sets(p, 0) && pools(p, false) && p.q8_filled.size() == 2);
        CHECK(!p.fft6_ready.holds("fc6") && !p.fft6_xf.holds("fc6") && !p.fft6_dyf.holds("fc6") && !p.fwd_v.holds("fc6"));
        CHECK(bwd_sets(p, 2) && p.dyg16_filled.size() == 2 && p.dgrad_v.holds("fc6") && p.dm.holds("fc6") && p.dm_prefilled.holds("fc6"));
        p = full(); p.begin_forward(true);
        CHECK(fwd_sets(p, 0) && p.q8_filled.empty() && bwd_sets(p, 2) && p.dyg16_filled.size() == 2);
    }
    {   // begin_backward: the backward facts, and of the hand-offs dm_prefilled alone
        PassState p = full(); p.begin_backward();
        CHECK(bwd_sets(p, 0) && p.dyg16_filled.empty() && !p.dm_prefilled.holds("fc6"));
        CHECK(fwd_sets(p, 2) && p.q8_filled.size() == 2 && pools(p, true) && p.fft6_ready.holds("fc6") && p.fft6_xf.holds("fc6"));
        CHECK(p.dm.holds("fc6") && p.dgrad_v.holds("fc6") && p.fwd_v.holds("fc6") && p.fft6_dyf.holds("fc6"));
    }
    {   // forget_shape_copies: the three "copy is filled" sets, nothing else; re-plans that keep the q8 copies keep their record
        PassState p = full(); p.forget_shape_copies(false);
        CHECK(p.xg16_filled.empty() && p.dyg16_filled.empty() && p.q8_filled.empty());
        CHECK(p.rbits_ok.size() == 2 && p.y_unwritten.size() == 2 && p.in_bf16_only.size() == 2 && bwd_sets(p, 2) && pools(p, true));
        for (Handoff* h : {&p.fft6_ready, &p.fft6_xf, &p.fwd_v, &p.dgrad_v, &p.dm, &p.dm_prefilled, &p.fft6_dyf}) CHECK(h->holds("fc6"));
        p = full(); p.forget_shape_copies(true);
        CHECK(p.xg16_filled.empty() && p.dyg16_filled.empty() && p.q8_filled.size() == 2);
    }
    {   // drop_backward_handoffs: dM and V in the shared scratch, nothing else
        PassState p = full(); p.drop_backward_handoffs();
        CHECK(!p.dm.holds("fc6") && !p.dgrad_v.holds("fc6"));
        CHECK(p.dm_prefilled.holds("fc6") && p.fft6_dyf.holds("fc6") && p.fwd_v.holds("fc6") && p.fft6_xf.holds("fc6") && p.fft6_ready.holds("fc6"));
        CHECK(fwd_sets(p, 2) && bwd_sets(p, 2) && p.dyg16_filled.size() == 2 && p.q8_filled.size() == 2 && pools(p, true));
    }
    std::puts("pass_state ok");
    return 0;
}
"""


def test_pass_state_rules_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "pass_state_main.cc"
    exe = tmp_path / "pass_state_main"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "fcn8s_tensorflow_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "pass_state ok", r.stdout + r.stderr
