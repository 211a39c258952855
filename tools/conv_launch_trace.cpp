// Host-dispatch trace of the convolution families without a GPU: links the host objects of csrc/conv_igemm.hip, conv_halo.hip,
// conv_subpixel.hip, conv_wgrad_slots.hip, conv_wgrad_subpixel.hip, conv1x1_stream.hip and gmk_common.hip with tools/launch_trace_stub.cpp
// (no libamdhip64) and prints one line per call of a sweep over their entry points: the return value, the gmk_last_error text (sticky, as in
// the library), gmk_last_kernel, and what the stand-in runtime saw - kernel name, grid, block, LDS bytes and the bytes of every kernel
// argument.  Every pointer is a distinct sentinel; no memory is touched.  Two builds whose traces are byte-identical dispatch identically.
//
//   hipcc <the Makefile's flags> -c csrc/<each of the seven>.hip
//   clang++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/conv_launch_trace.cpp tools/launch_trace_stub.cpp <the seven .o>
//   llvm-readelf --notes <code objects of the six: the hipcc line with --cuda-device-only --no-gpu-bundle-output> > notes.txt
//   LAUNCH_TRACE_NOTES=notes.txt ./a.out <entry point | all | switch | landmarks | plans> [mask]
//
// `switch` is the part of the sweep that GMK_SUBPIXEL reaches (the value is cached: run it once per value, each in a process of its own).
// `landmarks` prints the rows tests/test_host_logic.py asserts.  `plans` reads "halo B H W cu variant fold" / "slot B H W cout ktot stride2 cu forced" lines from
// stdin and prints what the planners of csrc/conv_plan.h return for them.  `mask` (for comparing with a tree from before the parameter structs were
// value-initialised) prints "--" for the fields such a tree leaves unset; the padding bytes of the structs print as "--" always.
// A stand-alone CPU program: not part of the library build, not a shared library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/gmk.h"
#if __has_include("../generative_models_amd/csrc/conv_plan.h")
#include "../generative_models_amd/csrc/conv_plan.h"
#define HAVE_PLANS 1
#endif

std::string launch_trace_take();      // launch_trace_stub.cpp
void launch_trace_mask(const char* kernel_part, size_t arg_size, size_t offset, size_t len);
void launch_trace_unmask(const char* kernel_part);

namespace {
template <typename T = void> T* ptr(int k) { return reinterpret_cast<T*>((uintptr_t)0x10000 * (uintptr_t)k); }      // sentinel number k
template <typename T = void> T* opt(bool on, int k) { return on ? ptr<T>(k) : nullptr; }
void* const kStream = ptr(99);
const int64_t kAmple = 1ll << 40;

struct Grid { int H, W; };
// the grids of tests/conv_ref.py's TABLE and SLOT_TABLE, the U-Net levels, and narrow / odd / too-wide ones (H x W of the OUTPUT)
const std::vector<Grid> kGrids = {{16, 16}, {28, 28}, {14, 14}, {8, 8}, {32, 32}, {64, 64}, {12, 20}, {10, 24}, {20, 12}, {7, 7},
                                  {7, 2}, {4, 4}, {5, 6}, {7, 6}, {4, 255}, {2, 254}, {2, 126}, {3, 128}, {62, 62}, {2, 4}, {1, 16}};
// one beyond each 32-bit limit: 4100 (bytes / 24-bit pixel indices at 64 x 64), 70000 (the same at 16 x 16), 600000 and 2^25 (31-bit pixel indices)
const std::vector<int> kB = {1, 2, 3, 9, 25, 37, 400, 2048, 4100, 70000, 600000, 1 << 25};
const std::vector<int> kBFew = {2, 25, 2048};
const std::vector<int> kCu = {8, 248, 256};
const std::vector<int> kChoice = {-1, 0, 1, 2, 3};            // GMK_CONV_KERNEL: -1 unset
const std::vector<int> kWChoice = {-1, 0, 1, 2};              // GMK_WGRAD_KERNEL
const std::vector<int> kDtype = {GMK_F32, GMK_BF16, GMK_F16, 7};
// every GMK_DEV_VARIANT value the six files compare against, host or device (302 = 46 + 256: the halo files mask to 8 bits, conv1x1_stream.hip does not)
const std::vector<int> kVariant = {0, 1, 3, 4, 6, 7, 8, 9, 11, 12, 13, 21, 22, 30, 32, 33, 46, 47, 61, 302};

void set_env(const char* name, int v) {
    if (v < 0) unsetenv(name);
    else setenv(name, std::to_string(v).c_str(), 1);
}
void set_switches(int conv, int wgrad, int cu) {
    gmk_set_kernel_choice(-1, -1, -1);
    set_env("GMK_CONV_KERNEL", conv); set_env("GMK_WGRAD_KERNEL", wgrad);
    gmk_set_cu_limit(cu);
}
void row(const char* entry, const char* what, long long rc) {
    printf("%s %s -> rc=%lld err=\"%s\" kernel=%d%s\n", entry, what, rc, gmk_last_error(), gmk_last_kernel(), launch_trace_take().c_str());
}
#define ROW(entry, call, ...)                      \
    do {                                           \
        char what[384];                            \
        snprintf(what, sizeof(what), __VA_ARGS__); \
        row(entry, what, call);                    \
    } while (0)

// ---- gmk_conv_igemm ----------------------------------------------------------------------------------------------------------------------
struct Conv {
    int c0 = 128, c1 = 0, cout = 128, n0 = 0, w_extra = 0, cs_extra = 0, ksize = 3, mode = GMK_CONV_NORMAL, dtype = GMK_F16;
    bool src1 = true, bias = true, emb = false, residual = false, stats = false, scale = false, shift = false, odd_src = false;
    int emb_stride = 512, gn_stride = 512;
    int64_t stats_bytes = kAmple;
};
void source_of(int mode, bool odd, int H, int W, int* hs, int* ws) {      // (H, W) is the output
    *hs = mode == GMK_CONV_STRIDE2 ? 2 * H - odd : mode == GMK_CONV_UPSAMPLE2 ? H / 2 : mode == GMK_CONV_TRANSPOSED2 ? (H - 1) / 2 + 1 : H;
    *ws = mode == GMK_CONV_STRIDE2 ? 2 * W - odd : mode == GMK_CONV_UPSAMPLE2 ? W / 2 : mode == GMK_CONV_TRANSPOSED2 ? (W - 1) / 2 + 1 : W;
}
void igemm(const Conv& c, int B, Grid g, const char* tag) {
    int hs, ws;
    source_of(c.mode, c.odd_src, g.H, g.W, &hs, &ws);
    ROW("conv_igemm", gmk_conv_igemm(ptr(1), opt(c.src1, 2), c.c0, c.c1, B, hs, ws, g.H, g.W, c.ksize, c.mode, ptr(3), c.n0 + c.cout + c.w_extra, c.n0, c.cout,
                                     opt<float>(c.bias, 4), opt<float>(c.emb, 5), c.emb_stride, opt(c.residual, 6), ptr(7), c.cout + c.cs_extra,
                                     opt<float>(c.stats, 8), c.stats_bytes, opt<float>(c.scale, 9), opt<float>(c.shift, 10), c.gn_stride, c.dtype, kStream),
        "%s dtype=%d mode=%d k=%d B=%d grid=%dx%d src=%dx%d c=%d+%d cout=%d n0=%d+%d cs=+%d opt=%d%d%d%d%d%d%d strides=%d,%d stats_bytes=%lld", tag, c.dtype,
        c.mode, c.ksize, B, g.H, g.W, hs, ws, c.c0, c.c1, c.cout, c.n0, c.w_extra, c.cs_extra, c.src1, c.bias, c.emb, c.residual, c.stats, c.scale, c.shift,
        c.emb_stride, c.gn_stride, (long long)c.stats_bytes);
}
// one axis at a time from the defaults, over every grid, the few batch sizes, the four gather modes and the three legal types
template <typename F> void igemm_vary(const char* tag, F&& change) {
    for (int dt : {GMK_F16, GMK_BF16, GMK_F32}) for (int mode : {0, 1, 2, 3}) for (Grid g : kGrids) for (int B : kBFew) {
        Conv c;
        c.dtype = dt; c.mode = mode;
        change(c);
        igemm(c, B, g, tag);
    }
}
void sweep_igemm(bool null_row) {
    for (int ch : kChoice) for (int cu : kCu) for (int dt : kDtype) for (int mode : {0, 1, 2, 3, 4}) for (int k : {3, 1}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(ch, -1, cu);
        Conv c;
        c.dtype = dt; c.mode = mode; c.ksize = k;
        char tag[64];
        snprintf(tag, sizeof(tag), "choice=%d cu=%d", ch, cu);
        igemm(c, B, g, tag);
    }
    set_switches(-1, -1, 256);
    igemm_vary("ksize", [](Conv& c) { c.ksize = 2; });
    igemm_vary("odd-source", [](Conv& c) { c.odd_src = true; });
    for (int c0 : {64, 256}) igemm_vary("c0", [&](Conv& c) { c.c0 = c0; });
    for (int c1 : {128, 256, 64}) igemm_vary("c1", [&](Conv& c) { c.c1 = c1; });
    igemm_vary("c1-256+256", [](Conv& c) { c.c0 = c.c1 = 256; });
    igemm_vary("c1-no-src1", [](Conv& c) { c.c1 = 128; c.src1 = false; });
    igemm_vary("cout", [](Conv& c) { c.cout = 256; });
    igemm_vary("cout-c1", [](Conv& c) { c.cout = 256; c.c1 = 128; });
    igemm_vary("n0", [](Conv& c) { c.n0 = 128; });
    igemm_vary("w_rows", [](Conv& c) { c.w_extra = 128; });
    igemm_vary("out_cstride", [](Conv& c) { c.cs_extra = 128; });
    igemm_vary("no-bias", [](Conv& c) { c.bias = false; });
    igemm_vary("emb", [](Conv& c) { c.emb = true; });
    igemm_vary("emb-short", [](Conv& c) { c.emb = true; c.emb_stride = 64; });
    igemm_vary("residual", [](Conv& c) { c.residual = true; });
    igemm_vary("stats", [](Conv& c) { c.stats = true; });
    igemm_vary("stats-strided", [](Conv& c) { c.stats = true; c.cs_extra = 128; });
    for (int B : kBFew) for (Grid g : kGrids) for (int d : {0, -1}) {      // statistics buffer exact and one byte short (the size is per tile)
        Conv c;
        c.stats = true;
        const int R = 256 / g.W > 0 ? 256 / g.W : 1;
        c.stats_bytes = ((int64_t)B * g.H + R - 1) / R * 8 * 2 * (c.cout / 4) * 2 * 4 + d;
        igemm(c, B, g, "stats-bytes");
    }
    igemm_vary("gn", [](Conv& c) { c.scale = c.shift = true; });
    igemm_vary("gn-two-sources", [](Conv& c) { c.scale = c.shift = true; c.c1 = 128; });
    igemm_vary("gn-no-shift", [](Conv& c) { c.scale = true; });
    igemm_vary("gn-short", [](Conv& c) { c.scale = c.shift = true; c.gn_stride = 64; });
    for (int split : {1, 0}) {      // both fp32 arithmetic modes (0 last: the default)
        gmk_set_fp32_exact(!split);
        for (int ch : kChoice) {
            set_switches(ch, -1, 256);
            igemm_vary(split ? "fp32-split" : "fp32-exact", [](Conv& c) { c.dtype = GMK_F32; });
        }
    }
    for (int v : kVariant) for (int cu : kCu) for (int res : {0, 1}) {
        set_switches(-1, -1, cu);
        gmk_set_dev_variant(v);
        char tag[64];
        snprintf(tag, sizeof(tag), "variant=%d cu=%d", v, cu);
        igemm_vary(tag, [&](Conv& c) { c.residual = res; });
        if (!res) igemm_vary(tag, [&](Conv& c) { c.stats = true; });
        if (!res) igemm_vary(tag, [&](Conv& c) { c.scale = c.shift = true; });
    }
    for (int64_t bytes : {(int64_t)512 * 8, kAmple}) for (int v : {0, 13, 32, 4}) for (int cu : kCu) for (int res : {0, 1}) {
        set_switches(-1, -1, cu);
        gmk_set_dev_variant(v);
        gmk_dev_set_stamp_buffer(ptr(90), bytes);
        char tag[64];
        snprintf(tag, sizeof(tag), "stamps=%lld variant=%d cu=%d", (long long)bytes, v, cu);
        igemm_vary(tag, [&](Conv& c) { c.residual = res; });
    }
    gmk_dev_set_stamp_buffer(nullptr, kAmple);
    gmk_set_dev_variant(0);
    set_switches(-1, -1, 256);
    if (null_row) { Conv c; ROW("conv_igemm", gmk_conv_igemm(ptr(1), nullptr, 128, 0, 2, 16, 16, 16, 16, 3, 0, nullptr, 128, 0, 128, nullptr, nullptr, 0, nullptr, ptr(7), 128, nullptr, 0, nullptr, nullptr, 0, c.dtype, kStream), "null w"); }
}

void sweep_pair(bool null_row) {
    for (int ch : kChoice) for (int cu : kCu) for (int dt : kDtype) for (int c : {128, 256}) for (int v : {0, 46, 302}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(ch, -1, cu);
        gmk_set_dev_variant(v);
        ROW("conv1x1_pair", gmk_conv1x1_pair(ptr(1), c, B, g.H, g.W, ptr(3), 256, 0, ptr(7), ptr(11), dt, kStream), "choice=%d cu=%d dtype=%d c=%d variant=%d B=%d grid=%dx%d",
            ch, cu, dt, c, v, B, g.H, g.W);
    }
    gmk_set_dev_variant(0);
    set_switches(-1, -1, 256);
    for (int n0 : {128, 1}) for (int extra : {0, 128, -1}) for (int B : kBFew) for (Grid g : kGrids)
        ROW("conv1x1_pair", gmk_conv1x1_pair(ptr(1), 128, B, g.H, g.W, ptr(3), n0 + 256 + extra, n0, ptr(7), ptr(11), GMK_BF16, kStream), "n0=%d w_rows=%d B=%d grid=%dx%d", n0,
            n0 + 256 + extra, B, g.H, g.W);
    for (int split : {1, 0}) {
        gmk_set_fp32_exact(!split);
        for (int B : kBFew) for (Grid g : kGrids)
            ROW("conv1x1_pair", gmk_conv1x1_pair(ptr(1), 128, B, g.H, g.W, ptr(3), 256, 0, ptr(7), ptr(11), GMK_F32, kStream), "fp32-split=%d B=%d grid=%dx%d", split, B, g.H, g.W);
    }
    if (null_row) ROW("conv1x1_pair", gmk_conv1x1_pair(ptr(1), 128, 2, 16, 16, ptr(3), 256, 0, ptr(7), nullptr, GMK_BF16, kStream), "null out_b");
}

void sweep_fusable() {
    for (int ch : kChoice) for (int cu : kCu) for (int c0 : {64, 128, 256}) for (int c1 : {0, 128, 256, 64}) for (int cout : {128, 256, 64}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(ch, -1, cu);
        ROW("conv_gn_fusable", gmk_conv_gn_fusable(B, g.H, g.W, c0, c1, cout), "choice=%d cu=%d B=%d grid=%dx%d c=%d+%d cout=%d", ch, cu, B, g.H, g.W, c0, c1, cout);
    }
    set_switches(-1, -1, 256);
}

// ---- the folded skip convolution -------------------------------------------------------------------------------------------------------------
int skipfold(int B, Grid g, int c0, int cs, int cout, int n0, int nsk0, int extra, int dt) {
    return gmk_conv3x3_skipfold(ptr(1), c0, B, g.H, g.W, ptr(3), n0 + cout + extra, n0, cout, ptr<float>(4), ptr(12), ptr(13), cs, ptr(14), nsk0 + cout + extra, nsk0,
                                ptr<float>(15), ptr(7), cout + extra, dt, kStream);
}
void sweep_skipfold(bool null_row) {
    for (int ch : kChoice) for (int cu : kCu) for (int dt : kDtype) for (int v : {0, 6, 8, 12, 4, 262}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(ch, -1, cu);
        gmk_set_dev_variant(v);
        ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 128, 0, 0, 0, dt), "choice=%d cu=%d dtype=%d variant=%d B=%d grid=%dx%d", ch, cu, dt, v, B, g.H, g.W);
    }
    gmk_set_dev_variant(0);
    set_switches(-1, -1, 256);
    for (Grid g : kGrids) for (int B : kBFew) {
        for (int c0 : {64, 256}) ROW("conv3x3_skipfold", skipfold(B, g, c0, 128, 128, 0, 0, 0, GMK_F16), "c0=%d B=%d grid=%dx%d", c0, B, g.H, g.W);
        ROW("conv3x3_skipfold", skipfold(B, g, 128, 256, 128, 0, 0, 0, GMK_F16), "cs=256 B=%d grid=%dx%d", B, g.H, g.W);
        ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 256, 0, 0, 0, GMK_F16), "cout=256 B=%d grid=%dx%d", B, g.H, g.W);
        ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 128, 128, 0, 0, GMK_F16), "n0=128 B=%d grid=%dx%d", B, g.H, g.W);
        ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 128, 0, 128, 0, GMK_F16), "nsk0=128 B=%d grid=%dx%d", B, g.H, g.W);
        ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 128, 0, 0, 128, GMK_F16), "rows-and-stride=+128 B=%d grid=%dx%d", B, g.H, g.W);
        ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 128, 0, 0, -1, GMK_F16), "rows-and-stride=-1 B=%d grid=%dx%d", B, g.H, g.W);
        for (int64_t bytes : {(int64_t)512 * 8, kAmple}) for (int v : {0, 12}) for (int cu : kCu) {
            set_switches(-1, -1, cu);
            gmk_set_dev_variant(v);
            gmk_dev_set_stamp_buffer(ptr(90), bytes);
            ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 128, 0, 0, 0, GMK_F16), "stamps=%lld variant=%d cu=%d B=%d grid=%dx%d", (long long)bytes, v, cu, B, g.H, g.W);
        }
        gmk_dev_set_stamp_buffer(nullptr, kAmple);
        gmk_set_dev_variant(0);
        set_switches(-1, -1, 256);
    }
    if (null_row)
        ROW("conv3x3_skipfold", gmk_conv3x3_skipfold(ptr(1), 128, 2, 16, 16, ptr(3), 128, 0, 128, ptr<float>(4), ptr(12), nullptr, 128, ptr(14), 128, 0, ptr<float>(15), ptr(7), 128,
                                                     GMK_F16, kStream), "null sk1");
}
void sweep_skipfold_ok() {
    for (int ch : kChoice) for (int cu : kCu) for (int c0 : {128, 64, 256}) for (int cs : {128, 256}) for (int cout : {128, 256}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(ch, -1, cu);
        ROW("conv3x3_skipfold_ok", gmk_conv3x3_skipfold_ok(B, g.H, g.W, c0, cs, cout), "choice=%d cu=%d B=%d grid=%dx%d c0=%d cs=%d cout=%d", ch, cu, B, g.H, g.W, c0, cs, cout);
    }
    set_switches(-1, -1, 256);
}

// ---- the sub-pixel forms ((H, W) is the LOW-resolution grid) -----------------------------------------------------------------------------------
void sweep_subpixel(const std::vector<int>& choices, bool null_row) {
    for (int ch : choices) for (int cu : kCu) for (int dt : kDtype) for (int mode : {0, 1, 2, 3}) for (int res : {0, 1}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(ch, -1, cu);
        ROW("conv_subpixel", gmk_conv_subpixel(ptr(1), B, g.H, g.W, 128, ptr(3), 128, 0, 128, mode, ptr<float>(4), opt(res, 6), ptr(7), 128, dt, kStream),
            "choice=%d cu=%d dtype=%d mode=%d residual=%d B=%d grid=%dx%d", ch, cu, dt, mode, res, B, g.H, g.W);
    }
    set_switches(-1, -1, 256);
    for (int mode : {0, 1, 2}) for (Grid g : kGrids) for (int B : kBFew) {
        for (int cin : {64, 256}) ROW("conv_subpixel", gmk_conv_subpixel(ptr(1), B, g.H, g.W, cin, ptr(3), 128, 0, 128, mode, ptr<float>(4), nullptr, ptr(7), 128, GMK_F16, kStream),
                                      "cin=%d mode=%d B=%d grid=%dx%d", cin, mode, B, g.H, g.W);
        ROW("conv_subpixel", gmk_conv_subpixel(ptr(1), B, g.H, g.W, 128, ptr(3), 256, 0, 256, mode, ptr<float>(4), nullptr, ptr(7), 256, GMK_F16, kStream), "cout=256 mode=%d B=%d grid=%dx%d", mode, B, g.H, g.W);
        for (int n0 : {0, 128}) for (int extra : {128, -1})
            ROW("conv_subpixel", gmk_conv_subpixel(ptr(1), B, g.H, g.W, 128, ptr(3), n0 + 128 + extra, n0, 128, mode, nullptr, nullptr, ptr(7), 128 + extra, GMK_BF16, kStream),
                "n0=%d rows-and-stride=%+d no-bias mode=%d B=%d grid=%dx%d", n0, extra, mode, B, g.H, g.W);
    }
    if (null_row) ROW("conv_subpixel", gmk_conv_subpixel(ptr(1), 2, 16, 16, 128, ptr(3), 128, 0, 128, 0, ptr<float>(4), nullptr, nullptr, 128, GMK_F16, kStream), "null out");
}
void sweep_subpixel_ok(const std::vector<int>& choices) {
    for (int ch : choices) for (int cu : kCu) for (int dt : kDtype) for (int cin : {128, 64, 256}) for (int cout : {128, 256}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(ch, -1, cu);
        ROW("conv_subpixel_ok", gmk_conv_subpixel_ok(B, g.H, g.W, cin, cout, dt), "choice=%d cu=%d dtype=%d cin=%d cout=%d B=%d grid=%dx%d", ch, cu, dt, cin, cout, B, g.H, g.W);
    }
    set_switches(-1, -1, 256);
}

// ---- weight gradients ------------------------------------------------------------------------------------------------------------------------
struct Types { int dtype, x_dtype; };
const std::vector<Types> kLegal = {{GMK_F32, GMK_F32}, {GMK_BF16, GMK_BF16}, {GMK_BF16, GMK_F16}};
const std::vector<Types> kIllegal = {{GMK_F16, GMK_F16}, {7, 7}, {GMK_BF16, GMK_F32}, {GMK_F32, GMK_F16}, {GMK_BF16, 5}};
void wgrad(const char* tag, Types t, int mode, int k, int B, Grid g, int c0, int c1, int cout, int cs_extra, bool odd, int ws_kind) {
    int hs, ws;
    source_of(mode, odd, g.H, g.W, &hs, &ws);
    const int64_t exact = gmk_conv_wgrad_workspace_bytes((int64_t)B * g.H * g.W, k * k, cout, c0 + c1);
    const int64_t bytes = ws_kind == 0 ? kAmple : exact + (ws_kind == 1 ? 0 : -1);
    ROW("conv_wgrad", gmk_conv_wgrad(ptr(21), cout + cs_extra, ptr(1), ptr(2), c0, c1, B, hs, ws, g.H, g.W, k, mode, ptr<float>(22), cout, ptr(23), bytes, t.dtype, t.x_dtype, kStream),
        "%s dtype=%d x_dtype=%d mode=%d k=%d B=%d grid=%dx%d src=%dx%d c=%d+%d cout=%d dy_cstride=+%d workspace=%s", tag, t.dtype, t.x_dtype, mode, k, B, g.H, g.W, hs, ws, c0, c1,
        cout, cs_extra, ws_kind == 0 ? "ample" : ws_kind == 1 ? "exact" : "short");
}
void sweep_wgrad(bool null_row) {
    for (int ch : kWChoice) for (int cu : kCu) for (int mode : {0, 1, 2, 3, 4}) for (int k : {3, 1}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(-1, ch, cu);
        char tag[64];
        snprintf(tag, sizeof(tag), "wchoice=%d cu=%d", ch, cu);
        for (Types t : kLegal) for (int ws_kind : {0, 1, 2}) wgrad(tag, t, mode, k, B, g, 128, 0, 128, 0, false, ws_kind);
        for (Types t : kIllegal) wgrad(tag, t, mode, k, B, g, 128, 0, 128, 0, false, 0);
    }
    for (int ch : kWChoice) for (int cu : kCu) for (Types t : kLegal) for (int mode : {0, 1, 2}) for (int k : {3, 1}) for (Grid g : kGrids) for (int B : kBFew) for (int ws_kind : {0, 1, 2}) {
        set_switches(-1, ch, cu);
        char tag[64];
        snprintf(tag, sizeof(tag), "wchoice=%d cu=%d", ch, cu);
        for (int c0 : {64, 256}) wgrad(tag, t, mode, k, B, g, c0, 0, 128, 0, false, ws_kind);
        for (int c1 : {128, 256, 64}) wgrad(tag, t, mode, k, B, g, 128, c1, 128, 0, false, ws_kind);
        wgrad(tag, t, mode, k, B, g, 256, 256, 256, 0, false, ws_kind);      // cout 256 x ktot 512
        wgrad(tag, t, mode, k, B, g, 256, 0, 256, 0, false, ws_kind);        // cout 256 x ktot 256
        wgrad(tag, t, mode, k, B, g, 128, 0, 128, 128, false, ws_kind);
        wgrad(tag, t, mode, k, B, g, 128, 0, 128, 4096, false, ws_kind);
        wgrad(tag, t, mode, k, B, g, 128, 0, 128, 0, true, ws_kind);
    }
    set_switches(-1, -1, 256);
    for (int v : {0, 61, 47, 317, 7, 9, 21, 22}) for (Types t : kLegal) for (int mode : {0, 1, 2}) for (int k : {3, 1}) for (Grid g : kGrids) for (int B : kBFew) {
        gmk_set_dev_variant(v);
        char tag[64];
        snprintf(tag, sizeof(tag), "variant=%d", v);
        wgrad(tag, t, mode, k, B, g, 128, k == 1 ? 128 : 0, 128, 0, false, 0);
    }
    gmk_set_dev_variant(0);
    for (int split : {1, 0}) {
        gmk_set_fp32_exact(!split);
        for (int mode : {0, 1, 2}) for (int k : {3, 1}) for (Grid g : kGrids) for (int B : kBFew) wgrad(split ? "fp32-split" : "fp32-exact", kLegal[0], mode, k, B, g, 128, 0, 128, 0, false, 0);
    }
    for (Types t : kLegal) wgrad("ksize", t, 0, 2, 2, {16, 16}, 128, 0, 128, 0, false, 0);
    if (null_row)
        ROW("conv_wgrad", gmk_conv_wgrad(ptr(21), 128, ptr(1), nullptr, 128, 0, 2, 16, 16, 16, 16, 3, 0, ptr<float>(22), 128, nullptr, kAmple, GMK_BF16, GMK_F16, kStream), "null workspace");
}
void sweep_wgrad_bytes() {
    for (int cu : kCu) for (int taps : {9, 1, 0, 4}) for (int cout : {128, 256, 100}) for (int ktot : {128, 256, 512, 100}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(-1, -1, cu);
        ROW("conv_wgrad_workspace_bytes", gmk_conv_wgrad_workspace_bytes((int64_t)B * g.H * g.W, taps, cout, ktot), "cu=%d taps=%d cout=%d ktot=%d pixels=%lld", cu, taps, cout, ktot,
            (long long)B * g.H * g.W);
    }
    ROW("conv_wgrad_workspace_bytes", gmk_conv_wgrad_workspace_bytes(0, 9, 128, 128), "no pixels");
    set_switches(-1, -1, 256);
}
void sweep_wgrad_subpixel(const std::vector<int>& choices, bool null_row) {
    std::vector<Types> types = {{GMK_BF16, GMK_BF16}, {GMK_BF16, GMK_F16}, {GMK_F32, GMK_F32}, {GMK_F16, GMK_F16}, {GMK_BF16, 7}};
    for (int ch : choices) for (int cu : kCu) for (Types t : types) for (int cio : {128, 256, 64}) for (int extra : {0, 128, 4096, -1}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(-1, ch, cu);
        const int64_t exact = gmk_conv_wgrad_subpixel_workspace_bytes(B, g.H, g.W, cio, cio);
        for (int ws_kind : {0, 1, 2})
            ROW("conv_wgrad_subpixel", gmk_conv_wgrad_subpixel(ptr(21), cio + extra, ptr(1), B, g.H, g.W, cio, cio, ptr<float>(22), ptr(23), ws_kind == 0 ? kAmple : exact - (ws_kind == 2),
                                                               t.dtype, t.x_dtype, kStream),
                "wchoice=%d cu=%d dtype=%d x_dtype=%d c=%d dy_cstride=%+d B=%d grid=%dx%d workspace=%s", ch, cu, t.dtype, t.x_dtype, cio, extra, B, g.H, g.W,
                ws_kind == 0 ? "ample" : ws_kind == 1 ? "exact" : "short");
    }
    set_switches(-1, -1, 256);
    if (null_row) ROW("conv_wgrad_subpixel", gmk_conv_wgrad_subpixel(ptr(21), 128, nullptr, 2, 16, 16, 128, 128, ptr<float>(22), ptr(23), kAmple, GMK_BF16, GMK_F16, kStream), "null x");
}
void sweep_wgrad_subpixel_ok(const std::vector<int>& choices) {
    for (int ch : choices) for (int cu : kCu) for (int cin : {128, 256, 64}) for (int cout : {128, 256}) for (Grid g : kGrids) for (int B : kB) {
        set_switches(-1, ch, cu);
        ROW("conv_wgrad_subpixel_ok", gmk_conv_wgrad_subpixel_ok(B, g.H, g.W, cin, cout), "wchoice=%d cu=%d cin=%d cout=%d B=%d grid=%dx%d", ch, cu, cin, cout, B, g.H, g.W);
        ROW("conv_wgrad_subpixel_workspace_bytes", gmk_conv_wgrad_subpixel_workspace_bytes(B, g.H, g.W, cin, cout), "wchoice=%d cu=%d cin=%d cout=%d B=%d grid=%dx%d", ch, cu, cin, cout,
            B, g.H, g.W);
    }
    set_switches(-1, -1, 256);
}

// ---- weight packs ----------------------------------------------------------------------------------------------------------------------------
void sweep_packs(bool masked) {
    for (int split : {1, 0}) {
        gmk_set_fp32_exact(!split);
        for (int dt : kDtype) for (int k : {1, 3, 2}) for (int cout : {128, 3, 0}) for (int cin : {128, 4, 12}) for (int which : {1, 2, 3})
            ROW("pack_conv_weight", gmk_pack_conv_weight(ptr<float>(31), opt(which & 1, 32), opt(which & 2, 33), cout, cin, k, dt, kStream), "fp32-split=%d dtype=%d k=%d cout=%d cin=%d packs=%d",
                split, dt, k, cout, cin, which);
        for (int dt : kDtype) for (int count : {0, 1, 3, 40, 41}) for (int f16 : {0, 1, 2}) for (int bad : {0, 1}) {      // f16: no table, all zero, every third entry
            int w_off[41], pack_off[41], cout[41], cin[41], ksize[41], flags[41];
            for (int e = 0; e < 41; ++e) { w_off[e] = 1000 * e; pack_off[e] = 3000 * e; cout[e] = 128 + e; cin[e] = 4 + e; ksize[e] = e % 2 ? 1 : 3; flags[e] = f16 == 2 && e % 3 == 0; }
            if (bad) ksize[count > 0 ? (count - 1) % 41 : 0] = 2;
            if (masked)      // the entries past `count` of the five tables
                for (int tab = 0; tab < 5 && count >= 0 && count < 40; ++tab) launch_trace_mask("pack_weights_multi_kernel", 816, 4 + 160 * tab + 4 * count, 4 * (40 - count));
            ROW("pack_conv_weights_multi", gmk_pack_conv_weights_multi(ptr<float>(31), ptr(32), count, w_off, pack_off, cout, cin, ksize, f16 ? flags : nullptr, dt, kStream),
                "fp32-split=%d dtype=%d count=%d fwd_f16=%d bad-entry=%d", split, dt, count, f16, bad);
            if (masked) { launch_trace_unmask("pack_weights_multi_kernel"); launch_trace_mask("pack_weights_multi_kernel", 816, 804, 4); }
        }
    }
    for (int dt : kDtype) for (int dd : kDtype) for (int cout : {128, 0}) for (int cin : {128, 4}) for (int which : {1, 2, 3})
        ROW("pack_upsample_weight", gmk_pack_upsample_weight(ptr<float>(31), opt(which & 1, 32), opt(which & 2, 33), cout, cin, dt, dd, kStream), "dtype=%d dgrad_dtype=%d cout=%d cin=%d packs=%d",
            dt, dd, cout, cin, which);
    ROW("pack_conv_weight", gmk_pack_conv_weight(nullptr, ptr(32), ptr(33), 128, 128, 3, GMK_BF16, kStream), "null w");
    ROW("pack_conv_weights_multi", gmk_pack_conv_weights_multi(ptr<float>(31), nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, GMK_BF16, kStream), "null packs");
    ROW("pack_upsample_weight", gmk_pack_upsample_weight(ptr<float>(31), nullptr, nullptr, 128, 128, GMK_F16, GMK_BF16, kStream), "null packs");
}

// ---- the rows tests/test_host_logic.py asserts: C = 128, B = 2048, the U-Net's four resolutions ----------------------------------------------
void landmarks() {
    const int B = 2048;
    set_switches(-1, -1, 256);
    for (int S : {8, 16, 32, 64}) {
        const Grid g = {S, S}, half = {S / 2, S / 2};
        for (int dt : {GMK_F16, GMK_BF16, GMK_F32}) {
            Conv c;
            c.dtype = dt;
            igemm(c, B, g, "plain");
            c.residual = true; igemm(c, B, g, "residual");
            c.residual = false; c.c1 = 128; igemm(c, B, g, "two-sources");
            Conv s; s.dtype = dt; s.mode = GMK_CONV_STRIDE2; igemm(s, B, half, "stride2");
            Conv t; t.dtype = dt; t.mode = GMK_CONV_TRANSPOSED2; t.residual = true; igemm(t, B, g, "transposed");
            set_switches(2, -1, 256); igemm(t, B, g, "transposed-choice2"); set_switches(-1, -1, 256);
            Conv u; u.dtype = dt; u.mode = GMK_CONV_UPSAMPLE2; igemm(u, B, g, "upsample");
            ROW("conv_subpixel", gmk_conv_subpixel(ptr(1), B, S / 2, S / 2, 128, ptr(3), 128, 0, 128, GMK_SUBPIXEL_UPSAMPLE, ptr<float>(4), nullptr, ptr(7), 128, dt, kStream), "dtype=%d grid=%dx%d", dt, S, S);
            ROW("conv_subpixel_ok", gmk_conv_subpixel_ok(B, S / 2, S / 2, 128, 128, dt), "dtype=%d grid=%dx%d", dt, S, S);
            ROW("conv3x3_skipfold", skipfold(B, g, 128, 128, 128, 0, 0, 0, dt), "dtype=%d grid=%dx%d", dt, S, S);
            ROW("conv1x1_pair", gmk_conv1x1_pair(ptr(1), 128, B, S, S, ptr(3), 256, 0, ptr(7), ptr(11), dt, kStream), "dtype=%d grid=%dx%d", dt, S, S);
        }
        ROW("conv3x3_skipfold_ok", gmk_conv3x3_skipfold_ok(B, S, S, 128, 128, 128), "grid=%dx%d", S, S);
        ROW("conv_gn_fusable", gmk_conv_gn_fusable(B, S, S, 128, 0, 128), "grid=%dx%d", S, S);
        { Conv f; f.scale = f.shift = true; igemm(f, B, g, "gn"); }
        for (Types t : {kLegal[2], kLegal[0]}) {
            const int ws_kind = 0;
            wgrad("3x3", t, GMK_CONV_NORMAL, 3, B, g, 128, 0, 128, 0, false, ws_kind);
            wgrad("3x3-two-sources", t, GMK_CONV_NORMAL, 3, B, g, 128, 128, 128, 0, false, ws_kind);
            wgrad("stride2", t, GMK_CONV_STRIDE2, 3, B, half, 128, 0, 128, 0, false, ws_kind);
            wgrad("upsample", t, GMK_CONV_UPSAMPLE2, 3, B, g, 128, 0, 128, 0, false, ws_kind);
            wgrad("skip-1x1", t, GMK_CONV_NORMAL, 1, B, g, 128, 128, 128, 0, false, ws_kind);
        }
        ROW("conv_wgrad_subpixel_ok", gmk_conv_wgrad_subpixel_ok(B, S / 2, S / 2, 128, 128), "grid=%dx%d", S, S);
        ROW("conv_wgrad_subpixel", gmk_conv_wgrad_subpixel(ptr(21), 128, ptr(1), B, S / 2, S / 2, 128, 128, ptr<float>(22), ptr(23), kAmple, GMK_BF16, GMK_F16, kStream), "grid=%dx%d", S, S);
    }
}

#ifdef HAVE_PLANS
void plans() {
    char kind[16];
    while (scanf("%15s", kind) == 1) {
        if (!strcmp(kind, "halo")) {      // C = 128, one source, dense output; variant and fold reach the schedule only
            int B, H, W, cu, variant, fold;
            if (scanf("%d %d %d %d %d %d", &B, &H, &W, &cu, &variant, &fold) != 6) break;
            HaloGeometry g = {};
            int grid_x = 0, nfull = 0, nhalf = 0;
            const int ok = gmk_halo_geometry(B, H, W, 128, 0, 128, 128, 128, 1, 0, 0, &g);
            if (ok) gmk_halo_schedule(g.ntiles, cu, variant, fold != 0, &grid_x, &nfull, &nhalf);
            printf("halo B=%d H=%d W=%d cu=%d variant=%d fold=%d eligible=%d R=%d TP=%d slots=%d rows=%lld M=%lld ntiles=%lld nb0=%lld nb1=%lld nbw=%lld nbo=%lld grid=%d nfull=%d "
                   "nhalf=%d\n", B, H, W, cu, variant, fold, ok, g.R, g.TP, g.slots, (long long)g.rows_total, (long long)g.M, (long long)g.ntiles, (long long)g.nb0, (long long)g.nb1,
                   (long long)g.nbw, (long long)g.nbo, grid_x, nfull, nhalf);
        } else if (!strcmp(kind, "slot")) {      // forced: GMK_WGRAD_KERNEL (0: with the automatic choice's work floor)
            int B, H, W, cout, ktot, s2, cu, forced;
            if (scanf("%d %d %d %d %d %d %d %d", &B, &H, &W, &cout, &ktot, &s2, &cu, &forced) != 8) break;
            SlotPlan p;
            const int ok = gmk_wgrad_slot_plan(B, H, W, ktot, 0, cout, cout, forced, 0, true, s2, cu, &p);
            printf("slot B=%d H=%d W=%d cout=%d ktot=%d stride2=%d cu=%d forced=%d eligible=%d kernel=%d wide=%d share=%d auto=%d WE=%d RE=%d nchunks=%d ns_cu=%d ns=%d cps=%d "
                   "grid=%d,%d,%d nbdy=%lld nb0=%lld nb1=%lld slab_bytes=%lld\n", B, H, W, cout, ktot, s2, cu, forced, ok, p.kernel, p.wide, p.share, p.auto_ok, p.WE, p.RE, p.nchunks,
                   p.ns_cu, p.ns, p.cps, p.grid[0], p.grid[1], p.grid[2], (long long)p.nbdy, (long long)p.nb0, (long long)p.nb1, (long long)p.slab_bytes);
        } else break;
    }
}
#endif
}  // namespace

int main(int argc, char** argv) {
    const char* which = argc > 1 ? argv[1] : "all";
    const bool masked = argc > 2 && !strcmp(argv[2], "mask");
    auto is = [&](const char* name) { return !strcmp(which, "all") || !strcmp(which, name); };
    // padding bytes of the by-value parameter structs (x86-64 layout of the structs in the six files)
    for (const char* k : {"conv3x3_halo_kernel", "conv3x3_halo_ws_kernel"})
        for (size_t off : {76, 116, 180, 268}) launch_trace_mask(k, 280, off, 4);                                          // HaloParams
    for (const char* k : {"conv_igemm_kernel", "conv_igemm_dma_kernel"}) {                                                     // ConvParams (GatherParams at 28)
        launch_trace_mask(k, 232, 99, 1);
        for (size_t off : {124, 148, 172, 196, 228}) launch_trace_mask(k, 232, off, 4);
    }
    launch_trace_mask("conv_wgrad_kernel", 176, 12, 4); launch_trace_mask("conv_wgrad_kernel", 176, 119, 1); launch_trace_mask("conv_wgrad_kernel", 176, 172, 4);      // WgradParams (GatherParams at 48)
    for (const char* k : {"conv_wgrad_slots_kernel", "conv_wgrad_slots_ws_kernel"}) { launch_trace_mask(k, 120, 12, 4); launch_trace_mask(k, 120, 84, 4); }            // SlotParams
    for (size_t off : {12, 52, 84}) launch_trace_mask("conv_wgrad_subpixel_ws_kernel", 88, off, 4);                                                                      // SubWgradParams
    launch_trace_mask("pack_weights_multi_kernel", 816, 804, 4);                                                                                                        // PackTable
    if (masked) {
        // HaloParams.sk0 ... nbws (the folded skip convolution's fields) in every launch but the fold's (kSkip = false: ...Li<shape>ELb<fuse>ELb0E...):
        // only the kSkip code reads them
        for (const char* k : {"conv3x3_halo_kernel", "ELi16ELb0ELb0E", "ELi16ELb1ELb0E", "ELi32ELb0ELb0E", "ELi32ELb1ELb0E"}) launch_trace_mask(k, 280, 216, 52);
        // ConvParams.nb0 ... nbo in the register-staged kernel: buffer sizes of the LDS-DMA kernel's descriptors, which conv_igemm_kernel has none of
        launch_trace_mask("conv_igemm_kernel", 232, 212, 16);
    }
    if (!strcmp(which, "landmarks")) { landmarks(); return 0; }
#ifdef HAVE_PLANS
    if (!strcmp(which, "plans")) { plans(); return 0; }
#endif
    if (!strcmp(which, "switch")) {
        Conv t;
        t.mode = GMK_CONV_TRANSPOSED2;
        for (int ch : kChoice) for (int cu : kCu) for (int dt : kDtype) for (int res : {0, 1}) for (Grid g : kGrids) for (int B : kB) {
            set_switches(ch, -1, cu);
            t.dtype = dt; t.residual = res;
            char tag[64];
            snprintf(tag, sizeof(tag), "choice=%d cu=%d", ch, cu);
            igemm(t, B, g, tag);
        }
        sweep_subpixel({-1, 3}, false); sweep_subpixel_ok(kChoice); sweep_wgrad_subpixel({-1}, false); sweep_wgrad_subpixel_ok(kWChoice);
        return 0;
    }
    if (is("conv_igemm")) sweep_igemm(true);
    if (is("conv1x1_pair")) sweep_pair(true);
    if (is("conv_gn_fusable")) sweep_fusable();
    if (is("conv3x3_skipfold")) sweep_skipfold(true);
    if (is("conv3x3_skipfold_ok")) sweep_skipfold_ok();
    if (is("conv_subpixel")) sweep_subpixel(kChoice, true);
    if (is("conv_subpixel_ok")) sweep_subpixel_ok(kChoice);
    if (is("conv_wgrad")) sweep_wgrad(true);
    if (is("conv_wgrad_workspace_bytes")) sweep_wgrad_bytes();
    if (is("conv_wgrad_subpixel")) sweep_wgrad_subpixel(kWChoice, true);
    if (is("conv_wgrad_subpixel_ok")) sweep_wgrad_subpixel_ok(kWChoice);
    if (is("packs")) sweep_packs(masked);
    return 0;
}
