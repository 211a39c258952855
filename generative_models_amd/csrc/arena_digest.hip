// gmk_arena_digest: a 64-bit, order-independent digest of a buffer of 4-byte words (no reference call site: an extension, used by
// checkpoint.py to tie model.pt to train_state.pt, to compare data-parallel replicas and to compare arenas without a host copy).
//
//   digest = sum over i of mix(w_i + (i + 1) * 0x9E3779B97F4A7C15)   (uint64, mod 2^64; w_i: the raw bits of word i; mix: splitmix64's finaliser)
//
// The sum is commutative and exact, so ANY split of the words over lanes, workgroups and passes gives the same 64 bits: the grid is a
// function of n_words alone (never of the CU limit), every workgroup adds its share into `out` with one 64-bit atomic add, and the entry zeroes
// `out` on the same stream first.  The index term makes the digest depend on WHERE a word sits: swapping two unequal words changes it.
//
// Layout of the work.  `data` is 4-byte aligned; `head` (0..3) words bring it to a 16-byte boundary, then `nq` quads of 4 words are read as one
// 16-byte load per lane in a grid-stride loop, then `tail` (0..3) words remain.  The at most 6 head and tail words go to lanes 0..5 of workgroup 0.
// Inside the loop the index term of a lane's quad is stepped by ADDING gridDim * 256 * 4 * K per pass (one 64-bit multiply per lane in front of
// the loop, none in it besides mix's own two).
#include "gmk_common.h"

namespace {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kDigestThreads = 256;
constexpr int kDigestMaxBlocks = 1024;      // one pass of the full grid covers 1024 * 256 quads = 2^20 words

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// words: 4-byte aligned; words + head: 16-byte aligned; n = head + 4 nq + tail
__global__ __launch_bounds__(kDigestThreads) void arena_digest_kernel(const uint32_t* __restrict__ words, int64_t n, int head, int64_t nq,
                                                                     unsigned long long* __restrict__ out) {
    __shared__ uint64_t red[kDigestThreads];
    const u32x4* __restrict__ quads = reinterpret_cast<const u32x4*>(words + head);
    const int64_t stride = (int64_t)gridDim.x * kDigestThreads;
    int64_t q = (int64_t)blockIdx.x * kDigestThreads + threadIdx.x;
    uint64_t term = ((uint64_t)(head + 4 * q) + 1) * kGolden;            // (i + 1) K of the quad's first word
    const uint64_t term_step = (uint64_t)(4 * stride) * kGolden;
    uint64_t acc = 0;
    for (; q < nq; q += stride, term += term_step) {
        const u32x4 w = quads[q];
        acc += mix64(w[0] + term);
        acc += mix64(w[1] + (term + kGolden));
        acc += mix64(w[2] + (term + 2 * kGolden));
        acc += mix64(w[3] + (term + 3 * kGolden));
    }
    if (blockIdx.x == 0) {                                                  // the words in front of the first quad and behind the last
        const int64_t body_end = head + 4 * nq;
        const int ntail = (int)(n - body_end);
        const int t = threadIdx.x;
        if (t < head + ntail) {
            const int64_t i = t < head ? t : body_end + (t - head);
            acc += mix64(words[i] + ((uint64_t)i + 1) * kGolden);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int half = kDigestThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(out, (unsigned long long)red[0]);
}

}  // namespace

extern "C" int gmk_arena_digest(const void* data, int64_t n_words, uint64_t* out, void* stream) {
    GMK_REQUIRE(data && out, "gmk_arena_digest: null pointer");
    GMK_REQUIRE(n_words > 0, "gmk_arena_digest: n_words = %lld must be positive", (long long)n_words);
    GMK_REQUIRE(((uintptr_t)data & 3) == 0, "gmk_arena_digest: data is not 4-byte aligned");
    GMK_REQUIRE(((uintptr_t)out & 7) == 0, "gmk_arena_digest: out is not 8-byte aligned");
    const int64_t to_boundary = (int64_t)(((16 - ((uintptr_t)data & 15)) & 15) / 4);
    const int head = (int)(to_boundary < n_words ? to_boundary : n_words);
    const int64_t nq = (n_words - head) / 4;
    const int64_t want = (nq + kDigestThreads - 1) / kDigestThreads;
    const int blocks = (int)(want < 1 ? 1 : want > kDigestMaxBlocks ? kDigestMaxBlocks : want);
    hipStream_t s = gmk_stream(stream);
    if (hipMemsetAsync(out, 0, sizeof(uint64_t), s) != hipSuccess) {
        gmk_set_error("gmk_arena_digest: zeroing out failed");
        return GMK_ERR_ARG;
    }
    arena_digest_kernel<<<blocks, kDigestThreads, 0, s>>>(static_cast<const uint32_t*>(data), n_words, head, nq,
                                                         reinterpret_cast<unsigned long long*>(out));
    return gmk_check_launch("gmk_arena_digest");
}
