// Samples out of the process: fp32 images in [-1, 1] -> the bytes of a dataset file (gmk_to_uint8) or of a tiled picture in the scanline
// layout a PNG encoder deflates (gmk_image_grid), each in one launch, with the quantisation of the reference's `proc`
// (gms/diffusion/diffusion_model.py:92).  The mirror image of batch_gather.hip, and like it not a hot spot in bytes (4 bytes read and 1
// written per pixel, 3 written for grey shown as RGB); its value is the single pass - no full-size fp32 temporaries between the sample and
// its bytes - and the layout, which needs no host-side shuffle before zlib.
#include "gmk_common.h"

namespace {

// q(x) = (uint8) trunc(min(max((x + 1) * 127.5, 0), 255)): the add and the multiply round separately, as torch evaluates the chain (the
// library is built with -ffp-contract=off, and an add feeding a multiply has no fused form anyway).  The comparisons are written out so
// that NaN takes the `0` arm: NaN -> 0, -inf -> 0, +inf and overflow -> 255.
__device__ __forceinline__ uint32_t quantize(float x) {
    float v = (x + 1.0f) * 127.5f;
    v = v > 0.0f ? v : 0.0f;
    v = v < 255.0f ? v : 255.0f;
    return (uint32_t)v;
}

// four consecutive floats, as wide as the address allows (p is 4-byte aligned)
__device__ __forceinline__ void load_run4(const float* p, float (&v)[4]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if ((addr & 15) == 0) {
        load4(p, v);
    } else if ((addr & 7) == 0) {          // the pad32 crop: rows start 2 floats off the 16-byte groups
        const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}

// ---- gmk_to_uint8 ------------------------------------------------------------------------------------------------------------------------
struct U8Args {
    const float* x;
    uint8_t* out;
    int W, crop, w;
    int64_t hw_in;       // H W: floats of one source plane
    int64_t hw_out;      // h w: bytes of one output plane
    int64_t total;       // n C h w
};

// the source of output byte e
__device__ __forceinline__ const float* u8_source(const U8Args& a, int64_t e) {
    const int64_t p = e / a.hw_out;
    const int r = (int)(e - p * a.hw_out);
    const int oy = r / a.w, ox = r - oy * a.w;
    return a.x + p * a.hw_in + (int64_t)(oy + a.crop) * a.W + ox + a.crop;
}

// One thread per aligned 4-byte group of the flat output (out is 4-byte aligned, so every group is one dword store).  A group inside one
// output row reads four consecutive floats; one that crosses a row end, and the n C h w % 4 bytes of the tail, go element by element.
__global__ __launch_bounds__(256) void to_uint8_kernel(const U8Args a) {
    const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= a.total) return;
    if (e0 + 4 > a.total) {
        for (int64_t e = e0; e < a.total; ++e) a.out[e] = (uint8_t)quantize(*u8_source(a, e));
        return;
    }
    float v[4];
    const int ox = (int)((e0 % a.hw_out) % a.w);
    if (ox + 4 <= a.w) {
        load_run4(u8_source(a, e0), v);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = *u8_source(a, e0 + i);
    }
    *reinterpret_cast<uint32_t*>(a.out + e0) = quantize(v[0]) | (quantize(v[1]) << 8) | (quantize(v[2]) << 16) | (quantize(v[3]) << 24);
}

// ---- gmk_image_grid ----------------------------------------------------------------------------------------------------------------------
struct GridArgs {
    const float* x;
    uint8_t* out;
    int T, N, H, W, crop, h, w, ncol, gap, prefix, GH, GW;
    int groups;          // ceil(GW / 4): threads per scanline
    uint32_t fill;
    int64_t hw;          // H W
    int64_t row;         // prefix + GW OC: bytes of one scanline
};

// One thread per 4 pixels of one scanline: it owns those pixels' OC bytes each (and, for the first group of a row, the filter byte), so every
// output byte has one writer and every source float one reader.  Four pixels inside one image row are read as a run (16-byte loads where the
// address allows); a group that touches a gap, the border, an empty tile or the row's end goes pixel by pixel.  The 4 OC bytes are stored as
// OC dwords when their address is 4-byte aligned - never with an odd row length, on some rows only with the filter byte - and one by one
// otherwise.
template <int C, int OC>
__global__ __launch_bounds__(256) void image_grid_kernel(const GridArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)a.T * a.GH * a.groups) return;
    const int g = (int)(gid % a.groups);
    const int64_t line = gid / a.groups;                   // t GH + gy
    const int gy = (int)(line % a.GH);
    const int64_t t = line / a.GH;
    const int px0 = g * 4;
    const int npx = a.GW - px0 < 4 ? a.GW - px0 : 4;
    uint8_t* orow = a.out + line * a.row;
    if (g == 0 && a.prefix) orow[0] = 0;                   // PNG filter type "None"
    uint8_t* dst = orow + a.prefix + (int64_t)px0 * OC;

    uint32_t q[4][C];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) q[i][c] = a.fill;
    const int pitch_y = a.h + a.gap, pitch_x = a.w + a.gap;
    const int ty = gy / pitch_y;
    const int iy = gy - ty * pitch_y - a.gap;              // < 0: a gap or border line (the last one has ty = nrow)
    if (iy >= 0) {
        const int tx0 = px0 / pitch_x;
        const int ix0 = px0 - tx0 * pitch_x - a.gap;
        const int64_t line_off = (int64_t)(iy + a.crop) * a.W + a.crop;
        if (npx == 4 && ix0 >= 0 && ix0 + 4 <= a.w && ty * a.ncol + tx0 < a.N) {
            const float* src = a.x + ((t * a.N + ty * a.ncol + tx0) * C) * a.hw + line_off + ix0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float v[4];
                load_run4(src + c * a.hw, v);
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i][c] = quantize(v[i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int px = px0 + i;
                const int tx = px / pitch_x;
                const int ix = px - tx * pitch_x - a.gap;          // < w always; px < GW keeps tx < ncol wherever ix >= 0
                const int j = ty * a.ncol + tx;
                if (i < npx && ix >= 0 && j < a.N) {
                    const float* src = a.x + ((t * a.N + j) * C) * a.hw + line_off + ix;
#pragma unroll
                    for (int c = 0; c < C; ++c) q[i][c] = quantize(src[c * a.hw]);
                }
            }
        }
    }
    // the 4 OC bytes in output order: channels interleaved, a grey value repeated OC times
    uint32_t words[OC] = {};
#pragma unroll
    for (int b = 0; b < 4 * OC; ++b) words[b / 4] |= q[b / OC][C == 1 ? 0 : b % OC] << (8 * (b % 4));
    if (npx == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < OC; ++k) reinterpret_cast<uint32_t*>(dst)[k] = words[k];
    } else {
#pragma unroll
        for (int b = 0; b < 4 * OC; ++b)
            if (b < npx * OC) dst[b] = (uint8_t)(words[b / 4] >> (8 * (b % 4)));
    }
}

}  // namespace

extern "C" int gmk_to_uint8(const float* x, uint8_t* out, int64_t n_images, int C, int H, int W, int crop, void* stream) {
    GMK_REQUIRE(x && out, "gmk_to_uint8: null pointer");
    GMK_REQUIRE(n_images > 0 && C > 0 && H > 0 && W > 0, "gmk_to_uint8: n_images, C, H, W must be positive");
    GMK_REQUIRE(crop >= 0 && crop <= 1024 && 2 * crop < (H < W ? H : W), "gmk_to_uint8: crop = %d of %d x %d images", crop, H, W);
    GMK_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0, "gmk_to_uint8: x not 16-byte aligned");
    GMK_REQUIRE(reinterpret_cast<uintptr_t>(out) % 4 == 0, "gmk_to_uint8: out not 4-byte aligned");
    U8Args a;
    a.x = x; a.out = out; a.W = W; a.crop = crop; a.w = W - 2 * crop;
    a.hw_in = (int64_t)H * W;
    a.hw_out = (int64_t)(H - 2 * crop) * a.w;
    GMK_REQUIRE(a.hw_in < (int64_t)1 << 31, "gmk_to_uint8: a plane of %lld elements", (long long)a.hw_in);
    GMK_REQUIRE(n_images <= ((int64_t)1 << 40) / ((int64_t)C * a.hw_in), "gmk_to_uint8: %lld images of %d x %d x %d", (long long)n_images, C, H, W);
    a.total = n_images * C * a.hw_out;
    const int64_t blocks = ((a.total + 3) / 4 + 255) / 256;
    GMK_REQUIRE(blocks < (int64_t)1 << 31, "gmk_to_uint8: too large (%lld workgroups)", (long long)blocks);
    to_uint8_kernel<<<(unsigned)blocks, 256, 0, gmk_stream(stream)>>>(a);
    return gmk_check_launch("gmk_to_uint8");
}

extern "C" int gmk_image_grid(const float* x, uint8_t* out, int T, int N, int C, int H, int W, int crop, int ncol, int gap, int fill,
                              int out_channels, int row_prefix, void* stream) {
    GMK_REQUIRE(x && out, "gmk_image_grid: null pointer");
    GMK_REQUIRE(T > 0 && N > 0 && H > 0 && W > 0, "gmk_image_grid: T, N, H, W must be positive");
    GMK_REQUIRE(C == 1 || C == 3, "gmk_image_grid: C = %d (1 or 3)", C);
    GMK_REQUIRE(out_channels == C || (out_channels == 3 && C == 1), "gmk_image_grid: out_channels = %d with C = %d", out_channels, C);
    GMK_REQUIRE(crop >= 0 && crop <= 1024 && 2 * crop < (H < W ? H : W), "gmk_image_grid: crop = %d of %d x %d images", crop, H, W);
    GMK_REQUIRE(ncol > 0 && ncol <= 1 << 20, "gmk_image_grid: ncol = %d", ncol);
    GMK_REQUIRE(gap >= 0 && gap <= 1024, "gmk_image_grid: gap = %d", gap);
    GMK_REQUIRE(fill >= 0 && fill <= 255, "gmk_image_grid: fill = %d (a byte)", fill);
    GMK_REQUIRE(row_prefix == 0 || row_prefix == 1, "gmk_image_grid: row_prefix = %d (0 or 1)", row_prefix);
    GMK_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0, "gmk_image_grid: x not 16-byte aligned");
    GridArgs a;
    a.x = x; a.out = out; a.T = T; a.N = N; a.H = H; a.W = W; a.crop = crop; a.h = H - 2 * crop; a.w = W - 2 * crop;
    a.ncol = ncol; a.gap = gap; a.prefix = row_prefix; a.fill = (uint32_t)fill;
    const int64_t nrow = ((int64_t)N + ncol - 1) / ncol;
    const int64_t GH = gap + nrow * (a.h + gap), GW = gap + (int64_t)ncol * (a.w + gap);
    a.hw = (int64_t)H * W;
    a.row = row_prefix + GW * out_channels;
    GMK_REQUIRE(GH * a.row < (int64_t)1 << 31 && a.hw < (int64_t)1 << 31, "gmk_image_grid: a frame of %lld x %lld pixels", (long long)GH, (long long)GW);
    GMK_REQUIRE((int64_t)T * N <= ((int64_t)1 << 40) / (C * a.hw), "gmk_image_grid: %d x %d images of %d x %d x %d", T, N, C, H, W);
    a.GH = (int)GH; a.GW = (int)GW; a.groups = (int)((GW + 3) / 4);
    const int64_t blocks = ((int64_t)T * a.GH * a.groups + 255) / 256;
    GMK_REQUIRE(blocks < (int64_t)1 << 31, "gmk_image_grid: too large (%lld workgroups)", (long long)blocks);
    hipStream_t s = gmk_stream(stream);
    if (C == 3)
        image_grid_kernel<3, 3><<<(unsigned)blocks, 256, 0, s>>>(a);
    else if (out_channels == 3)
        image_grid_kernel<1, 3><<<(unsigned)blocks, 256, 0, s>>>(a);
    else
        image_grid_kernel<1, 1><<<(unsigned)blocks, 256, 0, s>>>(a);
    return gmk_check_launch("gmk_image_grid");
}
