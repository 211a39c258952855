// Host-dispatch trace of the stem / head convolutions without a GPU, in the manner of tools/conv_launch_trace.cpp: links the host objects of
// csrc/smallconv.hip and gmk_common.hip with tools/launch_trace_stub.cpp (no libamdhip64) and prints one line per call of a sweep over the six
// entry points - the return value, the gmk_last_error text, gmk_last_kernel, and every launch the stand-in runtime saw.  Every pointer is a
// distinct sentinel; no memory is touched.
//
//   hipcc <the Makefile's flags> -c csrc/smallconv.hip csrc/gmk_common.hip
//   clang++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/smallconv_launch_trace.cpp tools/launch_trace_stub.cpp <the two .o>
//   llvm-readelf --notes <code object of smallconv.hip> > notes.txt
//   LAUNCH_TRACE_NOTES=notes.txt ./a.out
//
// The sweep: every storage type an entry accepts, C = 128 / 256, 1 - 4 image channels, five grids, GMK_DEV_VARIANT 0 / 41 / 42, B = 2
// (1920 lines; tests/test_host_logic.py states the count).  A stand-alone CPU program: not part of the library build, not a shared library.
#include <cstdio>
#include <string>
#include <vector>

#include "../include/gmk.h"

std::string launch_trace_take();      // launch_trace_stub.cpp

namespace {
template <typename T = void> T* ptr(int k) { return reinterpret_cast<T*>((uintptr_t)0x10000 * (uintptr_t)k); }      // sentinel number k
void* const kStream = ptr(99);
struct Grid { int H, W; };
char g_case[96];
void row(const char* entry, int dtype, int rc) {
    printf("%s %s dtype=%d -> rc=%d err=\"%s\" kernel=%d%s\n", entry, g_case, dtype, rc, gmk_last_error(), gmk_last_kernel(), launch_trace_take().c_str());
}
}  // namespace

int main() {
    const int B = 2;
    const std::vector<int> all3 = {GMK_F32, GMK_BF16, GMK_F16}, grads = {GMK_F32, GMK_BF16};
    for (int v : {0, 41, 42}) for (int C : {128, 256}) for (int cs : {1, 2, 3, 4}) for (Grid g : std::vector<Grid>{{8, 8}, {6, 7}, {28, 28}, {32, 32}, {4, 136}}) {
        gmk_set_dev_variant(v);
        snprintf(g_case, sizeof(g_case), "variant=%d C=%d cs=%d B=%d grid=%dx%d", v, C, cs, B, g.H, g.W);
        for (int dt : all3) row("stem_fwd", dt, gmk_stem_fwd(ptr<float>(41), ptr<float>(42), ptr<float>(43), ptr(44), B, cs, g.H, g.W, C, dt, kStream));
        for (int dt : grads) row("stem_wgrad", dt, gmk_stem_wgrad(ptr<float>(41), ptr(45), ptr<float>(46), B, cs, g.H, g.W, C, dt, kStream));
        for (int dt : all3) row("head_fwd", dt, gmk_head_fwd(ptr(47), ptr<float>(42), ptr<float>(43), ptr<float>(48), B, cs, g.H, g.W, C, dt, kStream));
        for (int dt : grads) row("head_dgrad", dt, gmk_head_dgrad(ptr<float>(49), ptr<float>(42), ptr(50), B, cs, g.H, g.W, C, dt, kStream));
        for (int dt : all3) row("head_wgrad", dt, gmk_head_wgrad(ptr<float>(49), ptr(47), ptr<float>(46), B, cs, g.H, g.W, C, dt, kStream));
        for (int dt : all3) row("stem_dgrad", dt, gmk_stem_dgrad(ptr(45), ptr<float>(42), ptr<float>(51), B, cs, g.H, g.W, C, dt, kStream));
    }
    return 0;
}
