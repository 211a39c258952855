// Batch assembly for a device-resident dataset: gather by index, the reference's transform chain (gms/common.py:104-111), zero padding and
// a random horizontal flip, uint8 [N][C][H][W] -> fp32 [B][C][H + 2 pad][W + 2 pad], in one launch.  Not a hot spot in bytes (1 byte read
// and 4 written per pixel); its value is the per-step host gather and host-to-device copy it replaces.
#include "gmk_common.h"

namespace {

struct GatherArgs {
    const uint8_t* images;
    const uint8_t* labels;
    const int64_t* index;
    float* x;
    int64_t* y;
    int B, C, H, W, pad, Ho, Wo;
    int64_t chw;        // C H W: bytes of one source image
    int64_t nout;       // C Ho Wo: floats of one output image
    int binarize;
    float flip_p;
    uint64_t seed, offset;
};

// element b of gmk_rng_uniform(seed, offset) < p: the convention of label_drop_kernel (embed.hip)
__device__ __forceinline__ bool flipped(const GatherArgs& a, int b) {
    if (a.flip_p <= 0.f) return false;          // flip_p = 0 draws nothing
    uint32_t rnd[4];
    philox4x32(a.offset + (uint64_t)(b >> 2), a.seed, rnd);
    return u01(rnd[b & 3]) < a.flip_p;
}

// one output element by its flat index in x: the path of every shape whose output rows are not whole 16-byte groups, and of the tail
__device__ __forceinline__ float gather_one(const GatherArgs& a, const float* lut, int64_t e) {
    const int b = (int)(e / a.nout);
    int r = (int)(e - (int64_t)b * a.nout);
    const int ox = r % a.Wo; r /= a.Wo;
    const int oy = r % a.Ho;
    const int c = r / a.Ho;
    const int sy = oy - a.pad;
    int sx = ox - a.pad;
    if (sy < 0 || sy >= a.H || sx < 0 || sx >= a.W) return 0.f;          // the border is 0 for the [-1, 1] data too (:110-111)
    if (flipped(a, b)) sx = a.W - 1 - sx;
    return lut[a.images[a.index[b] * a.chw + ((int64_t)c * a.H + sy) * a.W + sx]];
}

// ROWS4: Wo % 4 == 0, so a thread's four outputs lie in one output row and (x being 16-byte aligned) form one aligned 16-byte store.
template <bool ROWS4>
__global__ __launch_bounds__(256) void batch_gather_kernel(const GatherArgs a) {
    // the transform of every byte value, by the arithmetic of the CPU chain: float32(u8) / 255 (a correctly rounded division), then the
    // threshold or 2 x - 1 (2 x is exact, so the subtraction rounds once, as on the host)
    __shared__ float lut[256];
    {
        const float v = __fdiv_rn((float)threadIdx.x, 255.0f);
        lut[threadIdx.x] = a.binarize ? (v > 0.5f ? 1.f : 0.f) : 2.f * v - 1.f;
    }
    __syncthreads();
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < a.B) a.y[gid] = (int64_t)a.labels[a.index[gid]];
    const int64_t total = (int64_t)a.B * a.nout;
    const int64_t e0 = gid * 4;
    if (e0 >= total) return;
    if (!ROWS4) {
        if (e0 + 4 <= total) {
            const f32x4 v = {gather_one(a, lut, e0), gather_one(a, lut, e0 + 1), gather_one(a, lut, e0 + 2), gather_one(a, lut, e0 + 3)};
            *reinterpret_cast<f32x4*>(a.x + e0) = v;
        } else {
            for (int64_t e = e0; e < total; ++e) a.x[e] = gather_one(a, lut, e);          // scalar tail: B C Ho Wo % 4 elements
        }
        return;
    }
    const int b = (int)(e0 / a.nout);
    int r = (int)(e0 - (int64_t)b * a.nout);
    const int ox = r % a.Wo; r /= a.Wo;
    const int oy = r % a.Ho;
    const int c = r / a.Ho;
    const int sy = oy - a.pad;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (sy >= 0 && sy < a.H) {
        const bool flip = flipped(a, b);
        const uint8_t* row = a.images + a.index[b] * a.chw + ((int64_t)c * a.H + sy) * a.W;
        const int sx = ox - a.pad;                                   // source column of output 0 before the mirror
        const int lo = flip ? a.W - 4 - sx : sx;                     // lowest of the four source columns
        if (lo >= 0 && lo + 4 <= a.W) {
            // four source bytes row[lo .. lo + 3], loaded as wide as the address allows: image starts are 4-byte aligned only when
            // C H W % 4 == 0, and with pad = 2 the row sits 2 bytes off the output's groups
            const uint8_t* p = row + lo;
            const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
            uint32_t w;
            if ((addr & 3) == 0) {
                w = *reinterpret_cast<const uint32_t*>(p);
            } else if ((addr & 1) == 0) {
                w = (uint32_t)*reinterpret_cast<const uint16_t*>(p) | ((uint32_t)*reinterpret_cast<const uint16_t*>(p + 2) << 16);
            } else {
                w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            }
            if (flip) w = __builtin_bswap32(w);
            v[0] = lut[w & 255]; v[1] = lut[(w >> 8) & 255]; v[2] = lut[(w >> 16) & 255]; v[3] = lut[w >> 24];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {                            // a group that touches the border
                const int s = sx + i;
                if (s >= 0 && s < a.W) v[i] = lut[row[flip ? a.W - 1 - s : s]];
            }
        }
    }
    *reinterpret_cast<f32x4*>(a.x + e0) = v;
}

}  // namespace

extern "C" int gmk_batch_gather(const uint8_t* images, const uint8_t* labels, const int64_t* index, int B, int64_t N, int C, int H, int W,
                                int pad, int binarize, float flip_p, uint64_t seed, uint64_t offset, float* x, int64_t* y, void* stream) {
    GMK_REQUIRE(images && labels && index && x && y, "gmk_batch_gather: null pointer");
    GMK_REQUIRE(B > 0 && N > 0 && C > 0 && H > 0 && W > 0, "gmk_batch_gather: B, N, C, H, W must be positive");
    GMK_REQUIRE(pad >= 0 && pad <= 1024, "gmk_batch_gather: pad = %d", pad);
    GMK_REQUIRE(binarize == 0 || binarize == 1, "gmk_batch_gather: binarize = %d (0 or 1)", binarize);
    GMK_REQUIRE(flip_p >= 0.f && flip_p <= 1.f, "gmk_batch_gather: flip_p = %g outside [0, 1]", (double)flip_p);
    GMK_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0, "gmk_batch_gather: x not 16-byte aligned");
    GMK_REQUIRE(reinterpret_cast<uintptr_t>(index) % 8 == 0 && reinterpret_cast<uintptr_t>(y) % 8 == 0,
                "gmk_batch_gather: index / y not 8-byte aligned");
    GatherArgs a;
    a.images = images; a.labels = labels; a.index = index; a.x = x; a.y = y;
    a.B = B; a.C = C; a.H = H; a.W = W; a.pad = pad; a.Ho = H + 2 * pad; a.Wo = W + 2 * pad;
    a.chw = (int64_t)C * H * W;
    a.nout = (int64_t)C * a.Ho * a.Wo;
    GMK_REQUIRE(a.nout < (int64_t)1 << 31, "gmk_batch_gather: an output image of %lld elements", (long long)a.nout);
    a.binarize = binarize; a.flip_p = flip_p; a.seed = seed; a.offset = offset;
    const int64_t total = (int64_t)B * a.nout;
    const int64_t threads = (total + 3) / 4 > B ? (total + 3) / 4 : B;          // one per 16-byte group, and at least one per label
    const int64_t blocks = (threads + 255) / 256;
    GMK_REQUIRE(blocks < (int64_t)1 << 31, "gmk_batch_gather: batch too large (%lld workgroups)", (long long)blocks);
    if (a.Wo % 4 == 0)
        batch_gather_kernel<true><<<(unsigned)blocks, 256, 0, gmk_stream(stream)>>>(a);
    else
        batch_gather_kernel<false><<<(unsigned)blocks, 256, 0, gmk_stream(stream)>>>(a);
    return gmk_check_launch("gmk_batch_gather");
}
