// Brute-force nearest neighbours of byte rows under the squared Euclidean distance, exact: d2(q, j) = sum_i (queries[q][i] - database[j][i])^2
// as an integer, the k smallest (d2, j) pairs per query in lexicographic order (include/gmk.h: gmk_nn_search_u8).  No reference call site.
//
// Arithmetic: bytes become signed by b ^ 0x80 (= b - 128; differences are unchanged), d2 = |q'|^2 + |x'|^2 - 2 q'.x', the dot product on
// v_mfma_i32_32x32x32_i8 with int32 accumulation (|q'.x'| <= 32768 * 128 * 128 = 2^29: exact).  The A and B fragments of a lane are the same
// 16 consecutive bytes of one row of a row-major [row][k] tile, so whatever order the instruction gives the 32 k values of a step to its
// lanes, A and B agree on it and the sum over k does not depend on it; what the kernel relies on is C/D alone: column = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), the map of every 32 x 32 form.
//
// Three launches: the queries' norms (u8_sqnorm_kernel, into the workspace), nn_search_kernel, nn_merge_kernel.
//   nn_search_kernel  one workgroup per slab of GMK_NN_SLAB database rows, looping over tiles of 128 queries.  Both tiles go through LDS in K-steps
//                     of 64 bytes (registers hold the next step's 16-byte groups while the MFMAs of this one run); the tail of D beyond a
//                     multiple of 64, and rows beyond N or Q, are zeros in the signed domain and add nothing.  Wave w owns queries 32 w .. 32 w + 31
//                     of the tile against all 128 rows: four 32 x 32 accumulators with the QUERY as the column, so a lane sees 64 distances of one
//                     query and keeps their 8 smallest keys (d2 << 32 | j) in registers - no cross-lane step.  Lanes l and l + 32 hold the same query
//                     over different rows: each writes its own list, so a slab leaves 2 lists of k keys per query, [Q][2 slabs][k] in the workspace.
//   nn_merge_kernel   one wave per query: every lane folds its share of the 2 slabs lists into 8 keys, then 6 rounds of pairwise merges in LDS.
// Keys are distinct (j is), so every minimum is unique and the result is a function of the inputs alone: no atomics, no order-dependent step.
// The slab is read from HBM once per call (its later query tiles find it in L2: 128 x D <= 4 MiB); the queries are re-read by every slab.
#include "gmk_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr int kTile = GMK_NN_SLAB;          // database rows of a slab = queries of a tile
constexpr int kStep = 64;                   // bytes of K per LDS stage
constexpr int kLdsRow = kStep + 16;         // LDS row pitch: 16-byte groups stay aligned, rows start 20 banks apart
constexpr int kKeep = GMK_NN_MAX_K;         // keys a lane keeps, whatever k is
constexpr uint64_t kEmpty = ~(uint64_t)0;   // above every key: d2 < 2^31

static_assert(kTile == 128 && kKeep == 8, "the wave layout below is written for 128 x 128 tiles and lists of 8");

// `key` into the ascending list t, dropping its largest entry
__device__ __forceinline__ void keep_smallest(uint64_t (&t)[kKeep], uint64_t key) {
    if (key < t[kKeep - 1]) {
        t[kKeep - 1] = key;
#pragma unroll
        for (int i = kKeep - 1; i > 0; --i) {
            const uint64_t lo = t[i - 1] < t[i] ? t[i - 1] : t[i];
            const uint64_t hi = t[i - 1] < t[i] ? t[i] : t[i - 1];
            t[i - 1] = lo; t[i] = hi;
        }
    }
}

// bytes [col, col + 16) of row `row` as signed values (b ^ 0x80); zeros beyond the row's D bytes and beyond the last row.
// VEC: D % 16 == 0 and a 16-byte aligned base, so a group lies inside its row or outside it as a whole.
template <bool VEC>
__device__ __forceinline__ i32x4 load_group(const uint8_t* base, int64_t nrows, int D, int64_t row, int col) {
    i32x4 v = {0, 0, 0, 0};
    if (row >= nrows || col >= D) return v;
    const uint8_t* p = base + row * (int64_t)D + col;
    if (VEC) {
        v = *reinterpret_cast<const i32x4*>(p);
        v ^= (int)0x80808080u;
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (col + i < D) v[i >> 2] |= (int)((uint32_t)(p[i] ^ 0x80) << (8 * (i & 3)));
    }
    return v;
}

// 64-lane integer sum, every lane ends with the total: the lane pairing of lanes_sum_from (gmk_common.h), on the bits
__device__ __forceinline__ int wave_sum_i32(int v) {
    float a = __builtin_bit_cast(float, v), b = a;
    halves_swap32(a, b); v = __builtin_bit_cast(int, a) + __builtin_bit_cast(int, b);
    a = __builtin_bit_cast(float, v); b = a;
    rows_swap16(a, b); v = __builtin_bit_cast(int, a) + __builtin_bit_cast(int, b);
    v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
    return v;
}

// out[j] = sum_i (rows[j][i] - 128)^2: one wave per row, four rows per workgroup
template <bool VEC>
__global__ __launch_bounds__(256) void u8_sqnorm_kernel(const uint8_t* rows, int64_t N, int D, int* out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;                                    // the whole wave
    const uint8_t* p = rows + row * (int64_t)D;
    int s = 0;
    if (VEC) {
        for (int c = lane * 16; c < D; c += 64 * 16) {
            const i32x4 v = *reinterpret_cast<const i32x4*>(p + c);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b = (int)(((uint32_t)v[i >> 2] >> (8 * (i & 3))) & 255u) - 128;
                s += b * b;
            }
        }
    } else {
        for (int c = lane; c < D; c += 64) {
            const int b = (int)p[c] - 128;
            s += b * b;
        }
    }
    s = wave_sum_i32(s);
    if (lane == 0) out[row] = s;
}

struct SearchArgs {
    const uint8_t* queries;
    const uint8_t* database;
    const int* q_sqnorm;
    const int* db_sqnorm;
    uint64_t* parts;            // [Q][nparts][k]
    int64_t Q, N, nparts;
    int D, k;
};

template <bool VEC>
__global__ __launch_bounds__(256, 2) void nn_search_kernel(const SearchArgs a) {          // two workgroups per CU: at most 256 registers, none spilled
    __shared__ __attribute__((aligned(16))) uint8_t lds_db[kTile * kLdsRow];
    __shared__ __attribute__((aligned(16))) uint8_t lds_q[kTile * kLdsRow];
    __shared__ int lds_xn[kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    if (tid < kTile) lds_xn[tid] = row0 + tid < a.N ? a.db_sqnorm[row0 + tid] : 0;          // visible after the first barrier of the K loop (D >= 1)
    // staging: a tile's K-step is 128 rows x 4 groups of 16 bytes; thread t takes groups t and t + 256
    const int srow[2] = {tid >> 2, (tid + 256) >> 2};
    const int scol = (tid & 3) * 16;
    // operands: lane (r = lane & 31, h = lane >> 5) reads bytes 16 h .. 16 h + 15 of each 32-byte half-step of row r of its block
    const int frag = (lane & 31) * kLdsRow + (lane >> 5) * 16;
    for (int64_t q0 = 0; q0 < a.Q; q0 += kTile) {
        i32x16 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][i] = 0;
        i32x4 rdb[2], rq[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            rdb[g] = load_group<VEC>(a.database, a.N, a.D, row0 + srow[g], scol);
            rq[g] = load_group<VEC>(a.queries, a.Q, a.D, q0 + srow[g], scol);
        }
        for (int k0 = 0; k0 < a.D; k0 += kStep) {
            __syncthreads();                                 // every wave has read the stage before
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                *reinterpret_cast<i32x4*>(lds_db + srow[g] * kLdsRow + scol) = rdb[g];
                *reinterpret_cast<i32x4*>(lds_q + srow[g] * kLdsRow + scol) = rq[g];
            }
            __syncthreads();
            if (k0 + kStep < a.D) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    rdb[g] = load_group<VEC>(a.database, a.N, a.D, row0 + srow[g], k0 + kStep + scol);
                    rq[g] = load_group<VEC>(a.queries, a.Q, a.D, q0 + srow[g], k0 + kStep + scol);
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const i32x4 qf = *reinterpret_cast<const i32x4*>(lds_q + wave * 32 * kLdsRow + frag + ks * 32);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const i32x4 xf = *reinterpret_cast<const i32x4*>(lds_db + m * 32 * kLdsRow + frag + ks * 32);
                    acc[m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xf, qf, acc[m], 0, 0, 0);          // A = database rows, B = queries
                }
            }
        }
        // acc[m][i] = q'.x' for the query q0 + 32 wave + (lane & 31) and the slab row 32 m + (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
        const int64_t q = q0 + wave * 32 + (lane & 31);
        const uint32_t qn = q < a.Q ? (uint32_t)a.q_sqnorm[q] : 0u;
        uint64_t top[kKeep];
#pragma unroll
        for (int i = 0; i < kKeep; ++i) top[i] = kEmpty;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = 32 * m + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                const int64_t j = row0 + r;
                // mod 2^32: the terms reach 2^31, the distance itself is below it
                const uint32_t d2 = qn + (uint32_t)lds_xn[r] - 2u * (uint32_t)acc[m][i];
                if (j < a.N) keep_smallest(top, ((uint64_t)d2 << 32) | (uint64_t)(uint32_t)j);
            }
        }
        if (q < a.Q) {
            uint64_t* out = a.parts + (q * a.nparts + (int64_t)blockIdx.x * 2 + (lane >> 5)) * a.k;
#pragma unroll
            for (int i = 0; i < kKeep; ++i)
                if (i < a.k) out[i] = top[i];
        }
    }
}

// the k smallest of a query's nparts lists: one 64-lane workgroup per query
__global__ __launch_bounds__(64) void nn_merge_kernel(const uint64_t* parts, int64_t per_query, int k, int* dist2_out, int* index_out) {
    __shared__ uint64_t lists[64][kKeep];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const uint64_t* p = parts + q * per_query;
    uint64_t top[kKeep];
#pragma unroll
    for (int i = 0; i < kKeep; ++i) top[i] = kEmpty;
    for (int64_t e = lane; e < per_query; e += 64) keep_smallest(top, p[e]);
    for (int s = 1; s < 64; s *= 2) {
#pragma unroll
        for (int i = 0; i < kKeep; ++i) lists[lane][i] = top[i];
        __syncthreads();
        if (lane % (2 * s) == 0) {                           // lists of lanes lane and lane + s -> top: the 8 smallest of two ascending lists
            int ia = 0, ib = 0;
#pragma unroll
            for (int o = 0; o < kKeep; ++o) {                // ia + ib == o <= 7: both stay inside their lists
                const uint64_t x = lists[lane][ia], y = lists[lane + s][ib];
                const bool first = x <= y;
                top[o] = first ? x : y;
                ia += first ? 1 : 0; ib += first ? 0 : 1;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kKeep; ++i)
            if (i < k) {
                dist2_out[q * k + i] = (int)(uint32_t)(top[i] >> 32);
                index_out[q * k + i] = (int)(uint32_t)top[i];
            }
    }
}

inline int64_t nn_slabs(int64_t N) { return (N + kTile - 1) / kTile; }
inline int64_t nn_norm_bytes(int64_t Q) { return (Q * 4 + 15) / 16 * 16; }
inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int launch_sqnorm(const uint8_t* rows, int64_t N, int D, int* out, void* stream) {
    const unsigned blocks = (unsigned)((N + 3) / 4);
    if (D % 16 == 0 && aligned16(rows))
        u8_sqnorm_kernel<true><<<blocks, 256, 0, gmk_stream(stream)>>>(rows, N, D, out);
    else
        u8_sqnorm_kernel<false><<<blocks, 256, 0, gmk_stream(stream)>>>(rows, N, D, out);
    return gmk_check_launch("gmk_u8_sqnorm");
}

}  // namespace

extern "C" int gmk_u8_sqnorm(const uint8_t* rows, int64_t N, int D, int* out, void* stream) {
    GMK_REQUIRE(rows && out, "gmk_u8_sqnorm: null pointer");
    GMK_REQUIRE(N >= 1 && N < (int64_t)1 << 31, "gmk_u8_sqnorm: N = %lld (1 .. 2^31 - 1)", (long long)N);
    GMK_REQUIRE(D >= 1 && D <= GMK_NN_MAX_D, "gmk_u8_sqnorm: D = %d (1 .. %d)", D, GMK_NN_MAX_D);
    GMK_REQUIRE(reinterpret_cast<uintptr_t>(out) % 4 == 0, "gmk_u8_sqnorm: out not 4-byte aligned");
    return launch_sqnorm(rows, N, D, out, stream);
}

extern "C" int64_t gmk_nn_search_workspace(int64_t Q, int64_t N, int k) {
    if (Q < 1 || Q >= (int64_t)1 << 31 || N < 1 || N >= (int64_t)1 << 31 || k < 1 || k > GMK_NN_MAX_K) return -1;
    return nn_norm_bytes(Q) + Q * 2 * nn_slabs(N) * k * 8;          // < 2^31 * 2^25 * 64 = 2^62
}

extern "C" int gmk_nn_search_u8(const uint8_t* queries, int64_t Q, const uint8_t* database, int64_t N, int D, const int* db_sqnorm, int k,
                                void* workspace, int64_t workspace_bytes, int* dist2_out, int* index_out, void* stream) {
    GMK_REQUIRE(queries && database && db_sqnorm && workspace && dist2_out && index_out, "gmk_nn_search_u8: null pointer");
    GMK_REQUIRE(Q >= 1 && Q < (int64_t)1 << 31, "gmk_nn_search_u8: Q = %lld (1 .. 2^31 - 1)", (long long)Q);
    GMK_REQUIRE(N >= 1 && N < (int64_t)1 << 31, "gmk_nn_search_u8: N = %lld (1 .. 2^31 - 1)", (long long)N);
    GMK_REQUIRE(D >= 1 && D <= GMK_NN_MAX_D, "gmk_nn_search_u8: D = %d (1 .. %d: beyond it a squared distance leaves int32)", D, GMK_NN_MAX_D);
    GMK_REQUIRE(k >= 1 && k <= GMK_NN_MAX_K && k <= N, "gmk_nn_search_u8: k = %d with N = %lld (1 .. %d, at most N)", k, (long long)N, GMK_NN_MAX_K);
    const int64_t need = gmk_nn_search_workspace(Q, N, k);
    GMK_REQUIRE(workspace_bytes >= need, "gmk_nn_search_u8: workspace of %lld bytes, Q = %lld, N = %lld, k = %d need %lld", (long long)workspace_bytes,
                (long long)Q, (long long)N, k, (long long)need);
    GMK_REQUIRE(aligned16(workspace), "gmk_nn_search_u8: workspace not 16-byte aligned");
    GMK_REQUIRE(reinterpret_cast<uintptr_t>(db_sqnorm) % 4 == 0 && reinterpret_cast<uintptr_t>(dist2_out) % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(index_out) % 4 == 0, "gmk_nn_search_u8: db_sqnorm / dist2_out / index_out not 4-byte aligned");
    SearchArgs a;
    a.queries = queries; a.database = database; a.db_sqnorm = db_sqnorm;
    a.q_sqnorm = static_cast<const int*>(workspace);
    a.parts = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + nn_norm_bytes(Q));
    a.Q = Q; a.N = N; a.nparts = 2 * nn_slabs(N); a.D = D; a.k = k;
    int rc = launch_sqnorm(queries, Q, D, static_cast<int*>(workspace), stream);
    if (rc) return rc;
    if (D % 16 == 0 && aligned16(queries) && aligned16(database))
        nn_search_kernel<true><<<(unsigned)nn_slabs(N), 256, 0, gmk_stream(stream)>>>(a);
    else
        nn_search_kernel<false><<<(unsigned)nn_slabs(N), 256, 0, gmk_stream(stream)>>>(a);
    rc = gmk_check_launch("gmk_nn_search_u8");
    if (rc) return rc;
    nn_merge_kernel<<<(unsigned)Q, 64, 0, gmk_stream(stream)>>>(a.parts, a.nparts * k, k, dist2_out, index_out);
    return gmk_check_launch("gmk_nn_search_u8 (merge)");
}
