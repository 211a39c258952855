// Host-dispatch trace of the stem / head convolutions without a GPU, in the manner of tools/conv_launch_trace.cpp: links the host objects of
// csrc/smallconv.hip and gmk_common.hip with tools/launch_trace_stub.cpp (no libamdhip64) and prints one line per call of a sweep over the six
// entry points - the return value, the gmk_last_error text, gmk_last_kernel, and every launch the stand-in runtime saw.  Every pointer is a
// distinct sentinel; no memory is touched.  It calls exported entry points only, so the same source builds against any revision of csrc/.
//
//   hipcc <the Makefile's flags> -c csrc/smallconv.hip csrc/gmk_common.hip
//   clang++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/smallconv_launch_trace.cpp tools/launch_trace_stub.cpp <the two .o>
//   llvm-readelf --notes <code object of smallconv.hip> > notes.txt
//   LAUNCH_TRACE_NOTES=notes.txt ./a.out all | limits
//
// all:    every storage type an entry accepts, C = 128 / 256, 1 - 4 image channels, five grids, GMK_DEV_VARIANT 0 / 41 / 42, B = 2, the default
//         CU limit (1920 lines; tests/test_host_logic.py states the count).
// limits: the same calls where the grids clamp and the eligibility rules flip: CU limit 8 / 248 / 256 x the sizes of kLimitSizes (the
//         resident-set clamps, the 1024-pixel blocks beyond 2^20 pixels, buffers at and beyond the 32-bit byte limit, 2^24 pixels, rows of
//         exactly 128 pixels, the matrix-core contraction's LDS budget at and below one band row, an image too wide for any kernel), an illegal
//         storage type (variant 0) and one null pointer per entry.  The weight-gradient lines carry blocks= gmk_*_wgrad_blocks(B H W).
// A stand-alone CPU program: not part of the library build, not a shared library.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/gmk.h"

std::string launch_trace_take();      // launch_trace_stub.cpp

namespace {
template <typename T = void> T* ptr(int k) { return reinterpret_cast<T*>((uintptr_t)0x10000 * (uintptr_t)k); }      // sentinel number k
void* const kStream = ptr(99);
struct Grid { int H, W; };
struct Size { int B, H, W; };
const std::vector<Size> kLimitSizes = {
    {2, 32, 32}, {9, 32, 32}, {1024, 32, 32}, {2048, 32, 32}, {8192, 32, 32}, {16383, 32, 32}, {16384, 32, 32}, {1024, 64, 64}, {4096, 64, 64},
    {2, 12, 128},           // W = 128: the last tiled width; 2 image channels: 11 band rows fit 124 KiB of LDS, 12 would fit 128 KiB
    {2, 2, 400},            // 3 image channels: not one band row fits the matrix-core contraction, one fits the VALU kernel
    {2, 1, 2048},           // too wide for the VALU contraction as well
    {479349, 5, 7}};        // 2^24 - 1 pixels: a 16-bit C = 128 tensor of exactly the byte limit
char g_case[128];
void row(const char* entry, int dtype, int rc) {
    printf("%s %s dtype=%d -> rc=%d err=\"%s\" kernel=%d%s\n", entry, g_case, dtype, rc, gmk_last_error(), gmk_last_kernel(), launch_trace_take().c_str());
}
// one line per entry and storage type; null_at: the entry (0 - 5) that gets a null pointer, -1 none
void six_entries(const std::vector<int>& all3, const std::vector<int>& grads, int B, int cs, int H, int W, int C, int null_at = -1) {
    auto fp = [&](int entry, int k) { return null_at == entry ? nullptr : ptr<float>(k); };
    for (int dt : all3) row("stem_fwd", dt, gmk_stem_fwd(fp(0, 41), ptr<float>(42), ptr<float>(43), ptr(44), B, cs, H, W, C, dt, kStream));
    for (int dt : grads) row("stem_wgrad", dt, gmk_stem_wgrad(ptr<float>(41), ptr(45), fp(1, 46), B, cs, H, W, C, dt, kStream));
    for (int dt : all3) row("head_fwd", dt, gmk_head_fwd(ptr(47), fp(2, 42), ptr<float>(43), ptr<float>(48), B, cs, H, W, C, dt, kStream));
    for (int dt : grads) row("head_dgrad", dt, gmk_head_dgrad(ptr<float>(49), fp(3, 42), ptr(50), B, cs, H, W, C, dt, kStream));
    for (int dt : all3) row("head_wgrad", dt, gmk_head_wgrad(ptr<float>(49), ptr(47), fp(4, 46), B, cs, H, W, C, dt, kStream));
    for (int dt : all3) row("stem_dgrad", dt, gmk_stem_dgrad(ptr(45), ptr<float>(42), fp(5, 51), B, cs, H, W, C, dt, kStream));
}
}  // namespace

int main(int argc, char** argv) {
    const std::vector<int> all3 = {GMK_F32, GMK_BF16, GMK_F16}, grads = {GMK_F32, GMK_BF16}, illegal = {7};
    if (argc > 1 && !strcmp(argv[1], "limits")) {
        for (int cu : {8, 248, 256}) for (int v : {0, 41, 42}) for (int C : {128, 256}) for (int cs : {1, 2, 3, 4}) for (Size s : kLimitSizes) {
            gmk_set_cu_limit(cu);
            gmk_set_dev_variant(v);
            const int64_t npix = (int64_t)s.B * s.H * s.W;
            snprintf(g_case, sizeof(g_case), "cu=%d variant=%d C=%d cs=%d B=%d grid=%dx%d blocks=%d,%d", cu, v, C, cs, s.B, s.H, s.W,
                     gmk_stem_wgrad_blocks(npix), gmk_head_wgrad_blocks(npix));
            six_entries(all3, grads, s.B, cs, s.H, s.W, C);
            if (v == 0) six_entries(illegal, illegal, s.B, cs, s.H, s.W, C);
        }
        gmk_set_cu_limit(256);
        gmk_set_dev_variant(0);
        for (int k = 0; k < 6; ++k) {
            snprintf(g_case, sizeof(g_case), "null=%d", k);
            six_entries({GMK_BF16}, {GMK_BF16}, 2, 3, 32, 32, 128, k);
        }
        return 0;
    }
    const int B = 2;
    for (int v : {0, 41, 42}) for (int C : {128, 256}) for (int cs : {1, 2, 3, 4}) for (Grid g : std::vector<Grid>{{8, 8}, {6, 7}, {28, 28}, {32, 32}, {4, 136}}) {
        gmk_set_dev_variant(v);
        snprintf(g_case, sizeof(g_case), "variant=%d C=%d cs=%d B=%d grid=%dx%d", v, C, cs, B, g.H, g.W);
        six_entries(all3, grads, B, cs, g.H, g.W, C);
    }
    return 0;
}
