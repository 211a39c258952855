// k-NN radii and ball counts of fp32 rows under the squared Euclidean distance (include/gmk.h: gmk_knn_radius_f32, gmk_ball_counts_f32):
// what metrics.manifold_metrics needs of two N x N distance matrices, without either matrix.  No reference call site.
//
// Arithmetic: d2(a, b) = the chain acc = fmaf(a[i] - b[i], a[i] - b[i], acc) over i = 0 .. D - 1 in ascending order, from acc = 0.  Every pair
// has its own accumulator and sees its D elements in that order whatever the tile, chunk or lane it lands in, so the value is a function of the
// two rows alone; (a - b)^2 == (b - a)^2 in fp32, so it is symmetric bit for bit.  Elements beyond D are staged as zeros in both operands:
// t = 0, fmaf(0, 0, acc) == acc (acc >= +0), the chain's bits do not change.  A direct difference: no |a|^2 + |b|^2 - 2 a.b, no MFMA form.
//
// One kernel body, knn_tile_kernel, two epilogues.  A workgroup of 256 threads owns a tile of kT = 64 rows (queries / the points as "row i")
// and walks the kT-column tiles of one slab of GMK_KNN_SLAB columns (balls / the points as "column j").  Both tiles go through LDS in chunks
// of 64 floats of D (row pitch 68 floats: 16-byte groups stay aligned, the 16 column rows a wave reads start 4 banks apart and cover all 64
// banks once; the 4 row rows it reads are broadcasts); with D <= 64 the row tile is staged once per workgroup.  The next stage's 16-byte
// groups are fetched into registers while this one is computed.  Thread (tx = tid & 15, ty = tid >> 4) holds the 4 x 4 pairs
// (rows ty + 16 i, columns tx + 16 j): 16 independent chains, 8 ds_read_b128 per 128 VALU instructions (one v_sub + one v_fma per pair element).
//   radius epilogue   the 64 x 64 tile of d2 goes to LDS (columns beyond N as +inf), thread (r = tid >> 2, q = tid & 3) folds 16 values of row r
//                     into its ascending list of 9 values; after the slab the 4 lists of a row are merged by one thread and the k + 1 smallest
//                     go to the workspace [slab][k + 1][N] (coalesced both here and in knn_merge_kernel: one thread per row over all slabs).
//                     Lists hold VALUES, so which of two equal values is dropped does not matter: no atomics, no order-dependent step.
//   counts epilogue   inside = d2 < r2[column] (strict; columns beyond M compare against -1, rows beyond Q are left out): per-row counts stay
//                     in registers over the slab, per-column counts are flushed per tile, both through int32 LDS atomics and then one int32
//                     global atomic per non-zero row / column and workgroup.  Integer adds commute: the counts are a function of the inputs.
// The grid (row tiles x slabs) is a function of N / (M, Q) alone; gmk_set_cu_limit does not enter.
#include "gmk_common.h"

namespace {

constexpr int kT = GMK_KNN_TILE;             // rows and columns of a tile
constexpr int kChunk = 64;                   // floats of D per LDS stage
constexpr int kPitch = kChunk + 4;           // LDS row pitch of the operand tiles
constexpr int kD2Pitch = kT + 1;             // LDS row pitch of the d2 tile
constexpr int kKeep = GMK_NN_MAX_K + 1;      // values a list keeps, whatever k is: the k + 1 smallest are among them
constexpr int kSlabTiles = GMK_KNN_SLAB / kT;
constexpr int kMaxGridY = 65535;

static_assert(kT == 64 && kChunk == 64 && GMK_KNN_SLAB % kT == 0, "the thread layout below is written for 64 x 64 tiles and 64-float chunks");
static_assert(4 * kKeep * kT <= kT * kD2Pitch, "the slab's lists are merged in the d2 tile's LDS");

// `v` into the ascending list t, dropping its largest entry
__device__ __forceinline__ void keep_smallest(float (&t)[kKeep], float v) {
    if (v < t[kKeep - 1]) {
        t[kKeep - 1] = v;
#pragma unroll
        for (int i = kKeep - 1; i > 0; --i) {
            const float lo = fminf(t[i - 1], t[i]), hi = fmaxf(t[i - 1], t[i]);
            t[i - 1] = lo; t[i] = hi;
        }
    }
}

// floats [col, col + 4) of row `row`; zeros beyond the row's D floats and beyond the last row.
// VEC: D % 4 == 0 and a 16-byte aligned base, so a group lies inside its row or outside it as a whole.
template <bool VEC>
__device__ __forceinline__ f32x4 load_group(const float* base, int64_t nrows, int D, int64_t row, int col) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row >= nrows || col >= D) return v;
    const float* p = base + row * (int64_t)D + col;
    if (VEC) {
        v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (col + i < D) v[i] = p[i];
    }
    return v;
}

struct KnnArgs {
    const float* rows;            // [nrows][D]: the points (radius), the queries (counts)
    const float* cols;            // [ncols][D]: the points (radius), the balls (counts)
    const float* r2;              // counts: [ncols]
    float* parts;                 // radius: [slabs][k + 1][nrows]
    int* q_count;                 // counts: [nrows] or null
    int* m_count;                 // counts: [ncols] or null
    int64_t nrows, ncols, slab0;  // slab0: the slab of blockIdx.y == 0
    int D, k;
};

template <bool VEC, bool COUNTS>
__global__ __launch_bounds__(256) void knn_tile_kernel(const KnnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds_a[kT * kPitch];
    __shared__ __attribute__((aligned(16))) float lds_b[kT * kPitch];
    __shared__ float lds_x[kT * kD2Pitch];                   // radius: the d2 tile, then the slab's lists; counts: 2 kT int32 counters
    int* const cnt_m = reinterpret_cast<int*>(lds_x);
    int* const cnt_q = cnt_m + kT;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kT;
    const int64_t slab = a.slab0 + blockIdx.y;
    const int64_t col_begin = slab * GMK_KNN_SLAB;
    const int64_t left = a.ncols - col_begin;                // >= 1: the host launches existing slabs only
    const int ntiles = left >= GMK_KNN_SLAB ? kSlabTiles : (int)((left + kT - 1) / kT);
    const int nchunks = (a.D + kChunk - 1) / kChunk;
    const bool a_resident = nchunks == 1;                    // the row tile is staged once
    const int nstages = ntiles * nchunks;
    if (COUNTS && tid < 2 * kT) cnt_m[tid] = 0;              // visible after the first barrier of the stage loop

    // staging: a tile's chunk is 64 rows x 16 groups of 4 floats; thread (tx, ty) takes group tx of rows ty + 16 u
    f32x4 ra[4], rb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        ra[u] = load_group<VEC>(a.rows, a.nrows, a.D, row0 + ty + 16 * u, 4 * tx);
        rb[u] = load_group<VEC>(a.cols, a.ncols, a.D, col_begin + ty + 16 * u, 4 * tx);
    }
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    float top[kKeep];                                        // radius: thread (r = tid >> 2, q = tid & 3), 16 columns of row r per tile
#pragma unroll
    for (int i = 0; i < kKeep; ++i) top[i] = INFINITY;
    int qc[4] = {0, 0, 0, 0};                                // counts: rows ty + 16 i over the slab

    int ct = 0, c = 0;                                       // this stage: column tile, chunk of D
    for (int s = 0; s < nstages; ++s) {
        __syncthreads();                                     // every wave has read the stage before
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *reinterpret_cast<f32x4*>(lds_b + (ty + 16 * u) * kPitch + 4 * tx) = rb[u];
            if (!a_resident || s == 0) *reinterpret_cast<f32x4*>(lds_a + (ty + 16 * u) * kPitch + 4 * tx) = ra[u];
        }
        __syncthreads();
        int nct = ct, nc = c + 1;
        if (nc == nchunks) { nc = 0; ++nct; }
        if (s + 1 < nstages) {
            const int64_t ncol0 = col_begin + (int64_t)nct * kT;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                rb[u] = load_group<VEC>(a.cols, a.ncols, a.D, ncol0 + ty + 16 * u, nc * kChunk + 4 * tx);
                if (!a_resident) ra[u] = load_group<VEC>(a.rows, a.nrows, a.D, row0 + ty + 16 * u, nc * kChunk + 4 * tx);
            }
        }
        const int dlim = a.D - c * kChunk < kChunk ? a.D - c * kChunk : kChunk;
        for (int d = 0; d < dlim; d += 4) {
            f32x4 av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = *reinterpret_cast<const f32x4*>(lds_a + (ty + 16 * i) * kPitch + d);
                bv[i] = *reinterpret_cast<const f32x4*>(lds_b + (tx + 16 * i) * kPitch + d);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)                      // ascending in D for every pair; beyond D both operands are zeros
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float t = av[i][e] - bv[j][e];
                        acc[i][j] = __builtin_fmaf(t, t, acc[i][j]);
                    }
        }
        if (nc == 0) {                                       // the tile's last chunk: acc[i][j] = d2(row ty + 16 i, column tx + 16 j)
            const int64_t col0 = col_begin + (int64_t)ct * kT;
            if (COUNTS) {
                int mc[4] = {0, 0, 0, 0};
                float r2v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) r2v[j] = col0 + tx + 16 * j < a.ncols ? a.r2[col0 + tx + 16 * j] : -1.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool row_ok = row0 + ty + 16 * i < a.nrows;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int in = (acc[i][j] < r2v[j] && row_ok) ? 1 : 0;
                        qc[i] += in; mc[j] += in;
                    }
                }
                if (a.m_count) {                             // uniform over the grid
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (mc[j]) atomicAdd(&cnt_m[tx + 16 * j], mc[j]);
                    __syncthreads();
                    if (tid < kT) {                          // zeroed again two barriers before the next tile adds to it
                        const int v = cnt_m[tid];
                        if (v) { atomicAdd(&a.m_count[col0 + tid], v); cnt_m[tid] = 0; }
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        lds_x[(ty + 16 * i) * kD2Pitch + tx + 16 * j] = col0 + tx + 16 * j < a.ncols ? acc[i][j] : INFINITY;
                __syncthreads();                             // the next write of lds_x is two barriers away
                const float* mine = lds_x + (tid >> 2) * kD2Pitch + (tid & 3) * 16;
#pragma unroll
                for (int t = 0; t < 16; ++t) keep_smallest(top, mine[t]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
        }
        ct = nct; c = nc;
    }

    if (COUNTS) {
        if (a.q_count) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (qc[i]) atomicAdd(&cnt_q[ty + 16 * i], qc[i]);
            __syncthreads();
            if (tid < kT && row0 + tid < a.nrows) {
                const int v = cnt_q[tid];
                if (v) atomicAdd(&a.q_count[row0 + tid], v);
            }
        }
    } else {
        __syncthreads();                                     // every thread has folded the last tile
#pragma unroll
        for (int i = 0; i < kKeep; ++i) lds_x[tid * kKeep + i] = top[i];          // row r's four lists: lds_x[36 r .. 36 r + 35]
        __syncthreads();
        if (tid < kT && row0 + tid < a.nrows) {
            float m[kKeep];
#pragma unroll
            for (int i = 0; i < kKeep; ++i) m[i] = INFINITY;
            for (int e = 0; e < 4 * kKeep; ++e) keep_smallest(m, lds_x[tid * 4 * kKeep + e]);
            float* out = a.parts + slab * (a.k + 1) * a.nrows + row0 + tid;
#pragma unroll
            for (int i = 0; i < kKeep; ++i)
                if (i <= a.k) out[(int64_t)i * a.nrows] = m[i];
        }
    }
}

// the (k + 1)-th smallest of a row's nlists = slabs (k + 1) values: one thread per row, parts [nlists][N]
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* parts, int64_t N, int64_t nlists, int k, float* r2_out) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    float top[kKeep];
#pragma unroll
    for (int i = 0; i < kKeep; ++i) top[i] = INFINITY;
    for (int64_t e = 0; e < nlists; ++e) keep_smallest(top, parts[e * N + row]);
    float out = top[0];
#pragma unroll
    for (int i = 1; i < kKeep; ++i)
        if (i == k) out = top[i];
    r2_out[row] = out;
}

inline int64_t knn_slabs(int64_t n) { return (n + GMK_KNN_SLAB - 1) / GMK_KNN_SLAB; }
inline int64_t knn_tiles(int64_t n) { return (n + kT - 1) / kT; }
inline bool aligned_to(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// every (row tile, slab) pair, at most kMaxGridY slabs per launch
template <bool COUNTS>
int launch_tiles(KnnArgs a, const char* what, void* stream) {
    const bool vec = a.D % 4 == 0 && aligned_to(a.rows, 16) && aligned_to(a.cols, 16);
    const int64_t slabs = knn_slabs(a.ncols);
    for (int64_t s0 = 0; s0 < slabs; s0 += kMaxGridY) {
        a.slab0 = s0;
        const dim3 grid((unsigned)knn_tiles(a.nrows), (unsigned)(slabs - s0 < kMaxGridY ? slabs - s0 : kMaxGridY));
        if (vec)
            knn_tile_kernel<true, COUNTS><<<grid, 256, 0, gmk_stream(stream)>>>(a);
        else
            knn_tile_kernel<false, COUNTS><<<grid, 256, 0, gmk_stream(stream)>>>(a);
        const int rc = gmk_check_launch(what);
        if (rc) return rc;
    }
    return 0;
}

inline bool knn_rows_ok(int64_t n) { return n >= 1 && n < (int64_t)1 << 31; }

}  // namespace

extern "C" int64_t gmk_knn_radius_workspace(int64_t N, int k) {
    if (!knn_rows_ok(N) || k < 1 || k > GMK_NN_MAX_K || k + 1 > N) return -1;
    return knn_slabs(N) * (k + 1) * N * 4;                   // < 2^21 * 9 * 2^31 * 4 < 2^58
}

extern "C" int gmk_knn_radius_f32(const float* pts, int64_t N, int D, int k, void* workspace, int64_t workspace_bytes, float* r2_out,
                                  void* stream) {
    GMK_REQUIRE(pts && workspace && r2_out, "gmk_knn_radius_f32: null pointer");
    GMK_REQUIRE(knn_rows_ok(N), "gmk_knn_radius_f32: N = %lld (1 .. 2^31 - 1)", (long long)N);
    GMK_REQUIRE(D >= 1 && D <= GMK_KNN_MAX_D, "gmk_knn_radius_f32: D = %d (1 .. %d)", D, GMK_KNN_MAX_D);
    GMK_REQUIRE(k >= 1 && k <= GMK_NN_MAX_K && k + 1 <= N, "gmk_knn_radius_f32: k = %d with N = %lld (1 .. %d, k + 1 at most N)", k, (long long)N,
                GMK_NN_MAX_K);
    const int64_t need = gmk_knn_radius_workspace(N, k);
    GMK_REQUIRE(workspace_bytes >= need, "gmk_knn_radius_f32: workspace of %lld bytes, N = %lld, k = %d need %lld", (long long)workspace_bytes,
                (long long)N, k, (long long)need);
    GMK_REQUIRE(aligned_to(pts, 4) && aligned_to(workspace, 4) && aligned_to(r2_out, 4), "gmk_knn_radius_f32: pts / workspace / r2_out not 4-byte aligned");
    KnnArgs a = {};
    a.rows = pts; a.cols = pts; a.parts = static_cast<float*>(workspace);
    a.nrows = N; a.ncols = N; a.D = D; a.k = k;
    const int rc = launch_tiles<false>(a, "gmk_knn_radius_f32", stream);
    if (rc) return rc;
    knn_merge_kernel<<<(unsigned)((N + 255) / 256), 256, 0, gmk_stream(stream)>>>(a.parts, N, knn_slabs(N) * (k + 1), k, r2_out);
    return gmk_check_launch("gmk_knn_radius_f32 (merge)");
}

extern "C" int gmk_ball_counts_f32(const float* balls, const float* r2, int64_t M, const float* queries, int64_t Q, int D, int* q_count,
                                   int* m_count, void* stream) {
    GMK_REQUIRE(balls && r2 && queries, "gmk_ball_counts_f32: null pointer");
    GMK_REQUIRE(knn_rows_ok(M) && knn_rows_ok(Q), "gmk_ball_counts_f32: M = %lld, Q = %lld (1 .. 2^31 - 1)", (long long)M, (long long)Q);
    GMK_REQUIRE(D >= 1 && D <= GMK_KNN_MAX_D, "gmk_ball_counts_f32: D = %d (1 .. %d)", D, GMK_KNN_MAX_D);
    GMK_REQUIRE(aligned_to(balls, 4) && aligned_to(r2, 4) && aligned_to(queries, 4) && aligned_to(q_count, 4) && aligned_to(m_count, 4),
                "gmk_ball_counts_f32: balls / r2 / queries / q_count / m_count not 4-byte aligned");
    if (!q_count && !m_count) return 0;
    hipError_t e = q_count ? hipMemsetAsync(q_count, 0, (size_t)Q * 4, gmk_stream(stream)) : hipSuccess;
    if (e == hipSuccess && m_count) e = hipMemsetAsync(m_count, 0, (size_t)M * 4, gmk_stream(stream));
    if (e != hipSuccess) {
        gmk_set_error("gmk_ball_counts_f32 (zeroing the counts): %s", hipGetErrorString(e));
        return (int)e;
    }
    KnnArgs a = {};
    a.rows = queries; a.cols = balls; a.r2 = r2; a.q_count = q_count; a.m_count = m_count;
    a.nrows = Q; a.ncols = M; a.D = D; a.k = 0;
    return launch_tiles<true>(a, "gmk_ball_counts_f32", stream);
}
