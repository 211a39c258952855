// Host-dispatch trace of csrc/gn_silu.hip without a GPU: links the host objects of gn_silu.hip and gmk_common.hip with
// tools/launch_trace_stub.cpp (no libamdhip64) and prints, for every call of a sweep over the file's eleven entry points, one line with the
// return code, the gmk_last_error text (sticky, as in the library), gmk_last_kernel, and what the stand-in runtime saw: kernel name, grid,
// block, dynamic LDS bytes, hipFuncSetAttribute calls and the bytes of every kernel argument.  Every pointer and integer argument is a
// distinct sentinel, so two arguments swapped show up.  Two builds whose traces are byte-identical dispatch identically.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -c csrc/gn_silu.hip csrc/gmk_common.hip        (the Makefile's flags)
//   clang++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/gn_launch_trace.cpp tools/launch_trace_stub.cpp gn_silu.o gmk_common.o
//   llvm-readelf --notes <code object: the hipcc line with --cuda-device-only --no-gpu-bundle-output> > notes.txt
//   LAUNCH_TRACE_NOTES=notes.txt ./a.out <entry point | all | landmarks | cases>
//
// `landmarks` prints the handful of rows tests/test_host_logic.py asserts (C = 128, 32 groups, the five sizes of the U-Net levels).
// `cases` reads one call per line from stdin (the case tables of tests/gn_ref.py) and prints its row:
//   <entry> <mode | -1> <dtype> <x_dtype> <HW> <C> <groups> <groups_b> <dropout p> <xadd> <dxsum> <producer stats> <B>
// entry: gn_silu_fwd, gn_stats, gn_silu_bwd, gn_silu_fwd_pair (groups, groups_b = the two consumers) or gn_silu_bwd_pair (up, down).
// A stand-alone CPU program: not part of the library build, not a shared library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/gmk.h"

std::string launch_trace_take();      // launch_trace_stub.cpp
void launch_trace_padding(size_t arg_size, size_t offset, size_t len);

namespace {
template <typename T = void> T* ptr(int k) { return reinterpret_cast<T*>((uintptr_t)0x10000 * (uintptr_t)k); }      // sentinel number k
void* const kStream = ptr(99);
const float kEps = 1.25e-5f;
const uint64_t kSeed = 0x5eed5eed5eedull, kOffset = 0x0ff5e70ff5e7ull;

struct Axes {
    std::vector<int> dtype, xtype, HW, C, groups, mode, B, choice3;      // xtype: 0 same, 1 fp16, 2 illegal; choice3: absent / bad / good
    std::vector<float> drop;
};
const Axes kFull = {{GMK_F32, GMK_BF16, GMK_F16, 7}, {0, 1, 2},
                    {16, 49, 64, 65, 144, 196, 256, 257, 512, 576, 784, 832, 833, 1024, 1025, 2304, 4096, 4097},
                    {8, 32, 64, 96, 128, 160, 192, 256, 264}, {32, 16, 8, -1, -2, -3, -6, 0, 7},      // -1 / -2 stand for C and C / 2 groups
                    {-1, 0, 1, 3, 4, 5, 6, 7, 8, 9, 106, 107}, {1, 3}, {0, 1, 2}, {0.f, 0.1f, 1.f}};        // 100 + m: m in GMK_GN_KERNEL instead
// the landmark rows: 16-bit (fp16 activations, bf16 gradients) and fp32
const Axes kLandmarks = {{GMK_F16, GMK_F32}, {0}, {64, 256, 784, 1024, 4096}, {128}, {32}, {-1}, {2}, {0}, {0.f}};

int groups_of(int g, int C) { return g == -1 ? C : g == -2 ? C / 2 : g; }
void set_mode(int m) {
    gmk_set_kernel_choice(-1, -1, m >= 100 ? -1 : m);
    if (m >= 100) setenv("GMK_GN_KERNEL", std::to_string(m - 100).c_str(), 1);
    else unsetenv("GMK_GN_KERNEL");
}
void row(const char* entry, const char* what, int rc) {
    printf("%s %s -> rc=%d err=\"%s\" kernel=%d%s\n", entry, what, rc, gmk_last_error(), gmk_last_kernel(), launch_trace_take().c_str());
}
#define ROW(entry, call, ...)                      \
    do {                                           \
        char what[256];                            \
        snprintf(what, sizeof(what), __VA_ARGS__); \
        row(entry, what, call);                    \
    } while (0)

// strides of the optional per-(sample, channel) tables: absent, too short, long enough
const float* opt_ptr(int choice, int k) { return choice ? ptr<float>(k) : nullptr; }
int opt_stride(int choice, int C) { return choice == 1 ? C - 8 : choice == 2 ? C + 24 : 0; }

void sweep_fwd(const Axes& a, bool null_row) {
    for (int m : a.mode) for (int dt : a.dtype) for (int HW : a.HW) for (int C : a.C) for (int g : a.groups)
        for (float p : a.drop) for (int st : a.choice3) for (int xa : a.choice3) for (int B : a.B) {
            set_mode(m);
            const int G = groups_of(g, C);
            ROW("gn_silu_fwd", gmk_gn_silu_fwd(ptr(1), ptr(2), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), B, HW, C, G, kEps,
                                               opt_ptr(st, 7), st == 1 ? 16 : 32, 11, p, kSeed, kOffset, opt_ptr(xa, 8), opt_stride(xa, C), dt, kStream),
                "mode=%d dtype=%d HW=%d C=%d G=%d drop=%g stats=%d xadd=%d B=%d", m, dt, HW, C, G, (double)p, st, xa, B);
        }
    if (null_row)
        ROW("gn_silu_fwd", gmk_gn_silu_fwd(ptr(1), nullptr, ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), 1, 256, 128, 32, kEps, nullptr, 0, 0, 0.f,
                                           0, 0, nullptr, 0, GMK_F16, kStream), "null y");
}

void sweep_stats(const Axes& a, bool null_row) {
    for (int m : a.mode) for (int dt : a.dtype) for (int HW : a.HW) for (int C : a.C) for (int g : a.groups)
        for (int tab : a.choice3) for (int xa : a.choice3) for (int B : a.B) {
            set_mode(m);
            const int G = groups_of(g, C);
            ROW("gn_stats", gmk_gn_stats(ptr(1), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), ptr<float>(12), ptr<float>(13),
                                         tab == 1 ? C - 8 : tab == 2 ? C + 40 : C, B, HW, C, G, kEps, opt_ptr(xa, 8), opt_stride(xa, C), dt, kStream),
                "mode=%d dtype=%d HW=%d C=%d G=%d tab=%d xadd=%d B=%d", m, dt, HW, C, G, tab, xa, B);
        }
    if (null_row)
        ROW("gn_stats", gmk_gn_stats(ptr(1), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), nullptr, ptr<float>(13), 128, 1, 256, 128, 32, kEps,
                                     nullptr, 0, GMK_F16, kStream), "null tab_scale");
}

int x_dtype_of(int xt, int dt) { return xt == 0 ? dt : xt == 1 ? GMK_F16 : 5; }

void sweep_bwd(const Axes& a, bool null_row) {
    for (int m : a.mode) for (int dt : a.dtype) for (int xt : a.xtype) for (int HW : a.HW) for (int C : a.C) for (int g : a.groups)
        for (float p : a.drop) for (int xa : a.choice3) for (int ds : a.choice3) for (int B : a.B) {
            set_mode(m);
            const int G = groups_of(g, C), xdt = x_dtype_of(xt, dt);
            ROW("gn_silu_bwd", gmk_gn_silu_bwd(ptr(21), ptr(1), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), ptr(22), ptr(23), ptr(24),
                                               ptr<float>(25), ptr<float>(26), const_cast<float*>(opt_ptr(ds, 27)), opt_stride(ds, C), B, HW, C, G, p, kSeed,
                                               kOffset, opt_ptr(xa, 8), opt_stride(xa, C), dt, xdt, kStream),
                "mode=%d dtype=%d x_dtype=%d HW=%d C=%d G=%d drop=%g xadd=%d dxsum=%d B=%d", m, dt, xdt, HW, C, G, (double)p, xa, ds, B);
        }
    if (null_row)
        ROW("gn_silu_bwd", gmk_gn_silu_bwd(ptr(21), ptr(1), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), nullptr, nullptr, nullptr, ptr<float>(25),
                                           ptr<float>(26), nullptr, 0, 1, 256, 128, 32, 0.f, 0, 0, nullptr, 0, GMK_BF16, GMK_F16, kStream), "null dx");
}

void sweep_pair_ok(const Axes& a) {
    for (int m : a.mode) for (int xdt : a.dtype) for (int gdt : a.dtype) for (int HW : a.HW) for (int C : a.C) for (int ga : a.groups) for (int gb : a.groups) {
        set_mode(m);
        ROW("gn_pair_ok", gmk_gn_pair_ok(HW, C, groups_of(ga, C), groups_of(gb, C), xdt, gdt),
            "mode=%d x_dtype=%d grad_dtype=%d HW=%d C=%d G=%d,%d", m, xdt, gdt, HW, C, groups_of(ga, C), groups_of(gb, C));
    }
}

void sweep_pair_fwd_ok(const Axes& a) {
    for (int m : a.mode) for (int dt : a.dtype) for (int HW : a.HW) for (int C : a.C) for (int ga : a.groups) for (int gb : a.groups) {
        set_mode(m);
        ROW("gn_pair_fwd_ok", gmk_gn_pair_fwd_ok(HW, C, groups_of(ga, C), groups_of(gb, C), dt), "mode=%d dtype=%d HW=%d C=%d G=%d,%d", m, dt, HW, C,
            groups_of(ga, C), groups_of(gb, C));
    }
}

void sweep_fwd_pair(const Axes& a, bool null_row) {
    for (int m : a.mode) for (int dt : a.dtype) for (int HW : a.HW) for (int C : a.C) for (int ga : a.groups) for (int gb : a.groups)
        for (int xa : a.choice3) for (int B : a.B) {
            set_mode(m);
            const int Ga = groups_of(ga, C), Gb = groups_of(gb, C);
            ROW("gn_silu_fwd_pair", gmk_gn_silu_fwd_pair(ptr(1), ptr(31), ptr(32), ptr<float>(33), ptr<float>(34), ptr<float>(35), ptr<float>(36), ptr<float>(37),
                                                         ptr<float>(38), ptr<float>(39), ptr<float>(40), B, HW, C, Ga, Gb, kEps, opt_ptr(xa, 8),
                                                         opt_stride(xa, C), dt, kStream),
                "mode=%d dtype=%d HW=%d C=%d G=%d,%d xadd=%d B=%d", m, dt, HW, C, Ga, Gb, xa, B);
        }
    if (null_row)
        ROW("gn_silu_fwd_pair", gmk_gn_silu_fwd_pair(ptr(1), ptr(31), ptr(32), ptr<float>(33), ptr<float>(34), ptr<float>(35), ptr<float>(36), ptr<float>(37),
                                                     nullptr, ptr<float>(39), ptr<float>(40), 1, 256, 128, 32, 16, kEps, nullptr, 0, GMK_F16, kStream), "null rstd_a");
}

void sweep_bwd_pair(const Axes& a, bool null_row) {
    for (int m : a.mode) for (int dt : a.dtype) for (int HW : a.HW) for (int C : a.C) for (int ga : a.groups) for (int gb : a.groups)
        for (int xa : a.choice3) for (int ds : a.choice3) for (int B : a.B) {
            set_mode(m);
            const int Ga = groups_of(ga, C), Gb = groups_of(gb, C);
            ROW("gn_silu_bwd_pair", gmk_gn_silu_bwd_pair(ptr(1), ptr(41), ptr(42), ptr<float>(43), ptr<float>(44), ptr<float>(45), ptr<float>(46), ptr<float>(47),
                                                         ptr<float>(48), Ga, ptr(51), ptr(52), ptr<float>(53), ptr<float>(54), ptr<float>(55), ptr<float>(56),
                                                         ptr<float>(57), ptr<float>(58), Gb, ptr(24), const_cast<float*>(opt_ptr(ds, 27)), opt_stride(ds, C), B,
                                                         HW, C, opt_ptr(xa, 8), opt_stride(xa, C), dt, kStream),
                "mode=%d x_dtype=%d HW=%d C=%d G=%d,%d xadd=%d dxsum=%d B=%d", m, dt, HW, C, Ga, Gb, xa, ds, B);
        }
    if (null_row)
        ROW("gn_silu_bwd_pair", gmk_gn_silu_bwd_pair(ptr(1), ptr(41), nullptr, ptr<float>(43), ptr<float>(44), ptr<float>(45), ptr<float>(46), ptr<float>(47),
                                                     ptr<float>(48), 32, ptr(51), ptr(52), ptr<float>(53), ptr<float>(54), ptr<float>(55), ptr<float>(56),
                                                     ptr<float>(57), ptr<float>(58), 16, ptr(24), nullptr, 0, 1, 256, 128, nullptr, 0, GMK_F16, kStream), "null dadd_up");
}

void sweep_small(const Axes& a, const char* which) {
    const bool all = !strcmp(which, "all");
    if (all || !strcmp(which, "cast16")) {
        for (int s : a.dtype) for (int d : a.dtype) for (long long n : {0ll, 8ll, 12ll, 2048ll * 8, 1ll << 24, 1ll << 33})
            ROW("cast16", gmk_cast16(ptr(61), ptr(62), n, s, d, kStream), "src=%d dst=%d n=%lld", s, d, n);
        ROW("cast16", gmk_cast16(ptr(61), nullptr, 64, GMK_F16, GMK_BF16, kStream), "null dst");
    }
    if (all || !strcmp(which, "chansum")) {
        for (int dt : a.dtype) for (int HW : a.HW) for (int C : a.C) for (int os : {1, 2}) for (int B : a.B)
            ROW("chansum", gmk_chansum(ptr(61), ptr<float>(63), opt_stride(os, C), B, HW, C, dt, kStream), "dtype=%d HW=%d C=%d stride=%d B=%d", dt, HW, C,
                opt_stride(os, C), B);
        ROW("chansum", gmk_chansum(nullptr, ptr<float>(63), 128, 1, 64, 128, GMK_BF16, kStream), "null x");
    }
    if (all || !strcmp(which, "colsum")) {
        for (int R : {0, 1, 7, 2048}) for (int C : {0, 8, 33, 128, 264}) for (long long st : {-8ll, 0ll, 24ll}) for (int acc : {0, 1})
            ROW("colsum", gmk_colsum(ptr<float>(64), C + st, ptr<float>(65), R, C, acc, kStream), "R=%d C=%d stride=%lld accumulate=%d", R, C, C + st, acc);
        ROW("colsum", gmk_colsum(ptr<float>(64), 128, nullptr, 4, 128, 0, kStream), "null out");
    }
    if (all || !strcmp(which, "sumpool2x2")) {
        for (int dt : a.dtype) for (int H : {0, 1, 7, 16, 1024}) for (int W : {1, 16, 1024}) for (int C : {8, 12, 128, 264}) for (int B : a.B)
            ROW("sumpool2x2", gmk_sumpool2x2(ptr(61), ptr(62), B, H, W, C, dt, kStream), "dtype=%d H=%d W=%d C=%d B=%d", dt, H, W, C, B);
        ROW("sumpool2x2", gmk_sumpool2x2(ptr(61), nullptr, 1, 4, 4, 8, GMK_BF16, kStream), "null y");
    }
}

// one call per stdin line; the three flags are 0 / 1 (absent / present with a row stride of C + 24)
int sweep_cases() {
    char line[512], entry[64];
    while (fgets(line, sizeof(line), stdin)) {
        int m, dt, xdt, HW, C, G, G2, xa, ds, st, B;
        float p;
        if (line[0] == '\n' || line[0] == '#') continue;
        if (sscanf(line, "%63s %d %d %d %d %d %d %d %f %d %d %d %d", entry, &m, &dt, &xdt, &HW, &C, &G, &G2, &p, &xa, &ds, &st, &B) != 13) {
            fprintf(stderr, "cases: cannot read \"%s\"\n", line);
            return 2;
        }
        xa = xa ? 2 : 0; ds = ds ? 2 : 0; st = st ? 2 : 0;
        set_mode(m);
        char what[256];
        snprintf(what, sizeof(what), "mode=%d dtype=%d x_dtype=%d HW=%d C=%d G=%d,%d drop=%g xadd=%d dxsum=%d stats=%d B=%d", m, dt, xdt, HW, C, G, G2, (double)p,
                 xa, ds, st, B);
        if (!strcmp(entry, "gn_silu_fwd"))
            row(entry, what, gmk_gn_silu_fwd(ptr(1), ptr(2), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), B, HW, C, G, kEps, opt_ptr(st, 7), 32, 11, p,
                                             kSeed, kOffset, opt_ptr(xa, 8), opt_stride(xa, C), dt, kStream));
        else if (!strcmp(entry, "gn_stats"))
            row(entry, what, gmk_gn_stats(ptr(1), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), ptr<float>(12), ptr<float>(13), C + 40, B, HW, C, G, kEps,
                                          opt_ptr(xa, 8), opt_stride(xa, C), dt, kStream));
        else if (!strcmp(entry, "gn_silu_bwd"))
            row(entry, what, gmk_gn_silu_bwd(ptr(21), ptr(1), ptr<float>(3), ptr<float>(4), ptr<float>(5), ptr<float>(6), ptr(22), ptr(23), ptr(24), ptr<float>(25),
                                             ptr<float>(26), const_cast<float*>(opt_ptr(ds, 27)), opt_stride(ds, C), B, HW, C, G, p, kSeed, kOffset, opt_ptr(xa, 8),
                                             opt_stride(xa, C), dt, xdt, kStream));
        else if (!strcmp(entry, "gn_silu_fwd_pair"))
            row(entry, what, gmk_gn_silu_fwd_pair(ptr(1), ptr(31), ptr(32), ptr<float>(33), ptr<float>(34), ptr<float>(35), ptr<float>(36), ptr<float>(37), ptr<float>(38),
                                                  ptr<float>(39), ptr<float>(40), B, HW, C, G, G2, kEps, opt_ptr(xa, 8), opt_stride(xa, C), dt, kStream));
        else if (!strcmp(entry, "gn_silu_bwd_pair"))
            row(entry, what, gmk_gn_silu_bwd_pair(ptr(1), ptr(41), ptr(42), ptr<float>(43), ptr<float>(44), ptr<float>(45), ptr<float>(46), ptr<float>(47), ptr<float>(48),
                                                  G, ptr(51), ptr(52), ptr<float>(53), ptr<float>(54), ptr<float>(55), ptr<float>(56), ptr<float>(57), ptr<float>(58), G2,
                                                  ptr(24), const_cast<float*>(opt_ptr(ds, 27)), opt_stride(ds, C), B, HW, C, opt_ptr(xa, 8), opt_stride(xa, C), xdt,
                                                  kStream));
        else {
            fprintf(stderr, "cases: unknown entry point \"%s\"\n", entry);
            return 2;
        }
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const char* which = argc > 1 ? argv[1] : "all";
    launch_trace_padding(48, 44, 4);      // GnFwdSide: five pointers and an int
    launch_trace_padding(72, 68, 4);      // GnBwdSide: eight pointers and an int
    const bool landmarks = !strcmp(which, "landmarks"), all = !strcmp(which, "all");
    if (!strcmp(which, "cases")) return sweep_cases();
    if (landmarks) {
        Axes a = kLandmarks, grads = kLandmarks, mixed = kLandmarks;
        grads.dtype = {GMK_F32};                    // same-typed x
        mixed.dtype = {GMK_BF16}; mixed.xtype = {1};      // bf16 gradients beside fp16 x
        sweep_fwd(a, false); sweep_stats(mixed, false); sweep_stats(a, false); sweep_bwd(mixed, false); sweep_bwd(grads, false);
        a.dtype = {GMK_BF16, GMK_F16};
        sweep_pair_ok(a); sweep_pair_fwd_ok(a);
        return 0;
    }
    const Axes& a = kFull;
    if (all || !strcmp(which, "gn_silu_fwd")) sweep_fwd(a, true);
    if (all || !strcmp(which, "gn_stats")) sweep_stats(a, true);
    if (all || !strcmp(which, "gn_silu_bwd")) sweep_bwd(a, true);
    if (all || !strcmp(which, "gn_pair_ok")) sweep_pair_ok(a);
    if (all || !strcmp(which, "gn_pair_fwd_ok")) sweep_pair_fwd_ok(a);
    if (all || !strcmp(which, "gn_silu_fwd_pair")) sweep_fwd_pair(a, true);
    if (all || !strcmp(which, "gn_silu_bwd_pair")) sweep_bwd_pair(a, true);
    sweep_small(a, which);
    return 0;
}
