// Launch plans of the convolution families: which kernel a call gets, with what grid and schedule.  Plain C++ (no HIP types): the
// planners here take shapes, storage types, the kernel-choice switches and the CU limit, touch no pointer and launch nothing, so
// tools/conv_launch_trace.cpp can print what they return on a machine without a GPU.  The .hip file named beside each one defines it and
// launches from it.  (The halo and 1x1-stream launchers pick their instantiation themselves, from the geometry and schedule below.)
// The kernel ids the launchers report (GMK_K_*) are those of include/gmk.h's GMK_KERNEL_TABLE.
#pragma once
#include <stdint.h>

#include "../../include/gmk.h"

// Buffers the kernels address with 32-bit byte offsets end below (kBadPix * bytes-per-pixel) mod 2^32 (>= 0xFFFFF000 for pixels of up to 4 KiB)
static inline bool gmk_fits32(int64_t bytes) { return bytes < 0xFFFF0000ll; }
// GMK_CONV_KERNEL values under which the LDS-halo family (halo, folded skip, sub-pixel) may run: 0 automatic, 3 forced
static inline bool gmk_halo_family_allowed(int conv_choice) { return conv_choice == 0 || conv_choice == 3; }
// Split count of a persistent weight-gradient grid as the CU limit sets it.  Workgroups that stream the same operands are `ns` block ids
// apart: a multiple of 8 keeps them on one XCD; a multiple of 4 (two XCDs) is taken when the CU limit of a data-parallel run (248) would
// otherwise leave more than 1 / 16 of the CUs without a workgroup (1.18 -> 1.25 PFLOP/s at 64 x 64)
static inline int gmk_xcd_splits(int ns) {
    if (ns >= 8) {
        const int all8 = ns & ~7, two = ns & ~3;
        ns = all8 * 16 < ns * 15 ? two : all8;
    }
    return ns < 1 ? 1 : ns;
}

// ---- the halo kernels (conv_halo.hip) ---------------------------------------------------------------------------------------------------
struct HaloGeometry { int R, TP, slots; int64_t rows_total, M, ntiles, nb0, nb1, nbw, nbo; };      // slots: halo slots a tile uses (<= 448)
// The ONE eligibility rule of the halo kernels: 1 if they take this problem (g filled, if given), else 0
int gmk_halo_geometry(int B, int H, int W, int c0, int c1, int w_rows, int cout, int out_cstride, int min_tiles, int upsample,
                      int fused_gn, HaloGeometry* g);

// Tile schedule of the wave-specialised kernels over min(ntiles, cu_limit) workgroups: tiles [0, nfull) run as whole jobs, the rest as nhalf
// half-channel jobs; variant: GMK_DEV_VARIANT & 0xFF (4, 6, 8 switch the half jobs off, see there); fold: the launch of the folded skip convolution
void gmk_halo_schedule(int64_t ntiles, int cu_limit, int variant, bool fold, int* grid_x, int* nfull, int* nhalf);
// Launches by that rule: returns 1 (8-compute-wave kernel) or 2 (wave-specialised kernel), 0 if the problem is not eligible
// (upsample: 1 nearest x2, 2 zero-stuffed x2 source)
int gmk_conv3x3_halo_try(const void* src0, const void* src1, int c0, int c1, int B, int H, int W, const void* w, int w_rows,
                         int n0, int cout, const float* bias, const float* emb, int emb_stride, const void* residual,
                         void* out, int out_cstride, int min_tiles, int upsample, float* stats, int64_t stats_bytes,
                         const float* gn_scale, const float* gn_shift, int gn_stride, int dtype, void* stream);

// ---- the sub-pixel kernels (conv_subpixel.hip) --------------------------------------------------------------------------------------------
bool gmk_subpixel_enabled(void);      // GMK_SUBPIXEL != 0 (read once)
// Geometry of the low-resolution tiling (the byte sizes are those of the LOW -> HIGH forms); 0 if the sub-pixel kernel does not take the problem
int gmk_subpixel_plan(int B, int H, int W, int cin, int cout, int w_rows, int ntaps, int out_cstride, HaloGeometry* g);
// 1 if gmk_conv_subpixel takes the EXACT launch a caller is about to make (its own weight-row count and output stride enter the byte limits)
int gmk_subpixel_takes(int conv_choice, bool subpixel_on, int B, int H, int W, int cin, int cout, int w_rows, int ntaps, int out_cstride, int dtype);

// ---- gmk_conv_igemm (conv_igemm.hip) ------------------------------------------------------------------------------------------------------
enum ConvRoute {
    GMK_ROUTE_SUBPIXEL,       // gmk_conv_subpixel, transposed form
    GMK_ROUTE_HALO,           // gmk_conv3x3_halo_try
    GMK_ROUTE_PHASES,         // four output-parity phases on the LDS-DMA kernel
    GMK_ROUTE_NEEDS_HALO,     // a fused GroupNorm-apply that the halo kernel did not take: an error
    GMK_ROUTE_DMA,            // conv_igemm_dma_kernel
    GMK_ROUTE_REG,            // conv_igemm_kernel
    GMK_ROUTE_TWO_CALLS       // the pair form of a problem too small for the LDS-DMA kernel: one call per output block
};
struct ConvCall {      // a validated gmk_conv_igemm call without its pointers
    int c0, c1, B, hs, ws, ho, wo, ksize, mode, w_rows, n0, cout, out_cstride, dtype;
    bool emb, out2, gn_stats, gn_scale, gn_shift;
    int gn_stride;
};
struct ConvRoutePlan {
    ConvRoute route;
    bool stuffed;                       // transposed gather onto an even grid: the zero-stuffed source of the halo kernel
    int halo_min_tiles, halo_upsample;  // what gmk_conv3x3_halo_try is asked with
    int64_t nb0, nb1, nbw, nbo;         // byte sizes of the LDS-DMA kernel's buffers (the im2col routes)
};
// conv_choice: GMK_CONV_KERNEL; subpixel_on: GMK_SUBPIXEL != 0
ConvRoutePlan gmk_conv_route(const ConvCall& c, int conv_choice, bool subpixel_on);

// ---- weight gradients ---------------------------------------------------------------------------------------------------------------------
// Common shape: ok, the kernel id, the split count (= slabs written), its grid and the slab bytes the launch needs
struct SlotPlan {      // conv_wgrad_slots.hip: 3x3 bf16 weight gradient over padded slots
    int kernel;                 // GMK_K_CONV_WGRAD_SLOTS (8 compute waves), ..._SLOTS_WS (wave-specialised) or ..._SLOTS_S2 (its stride-2 four-plane form)
    bool wide, share;           // 128-slot window (rows beyond 62 pixels); dY slot and X slot are the same pixel
    bool auto_ok;               // enough chunks per split for the automatic choice (else the im2col kernel unless forced)
    int WE, RE, nchunks;
    int ns_cu, ns, cps;         // splits as the CU limit sets them, after the work clamps; chunks per split
    int grid[3];
    int64_t nbdy, nb0, nb1, slab_bytes;
};
int gmk_wgrad_slots_nsplit(int cout, int ktot, int cu_limit);
// forced: GMK_WGRAD_KERNEL (0 automatic, 2 the 8-compute-wave kernel); stride2: (H, W) is the OUTPUT (= dY) size, the source is (2H, 2W)
int gmk_wgrad_slot_plan(int B, int H, int W, int c0, int c1, int cout, int dy_cstride, int forced, int upsample, bool x_f16, int stride2,
                        int cu_limit, SlotPlan* plan);
// Launches by gmk_wgrad_slot_plan: returns the number of slabs written, 0 if not eligible or the slab is short
int gmk_conv_wgrad_slots_try(const void* dy, int dy_cstride, const void* src0, const void* src1, int c0, int c1, int B, int H,
                             int W, int cout, float* slab, int64_t slab_bytes, int forced, int upsample, bool x_f16,
                             void* stream, int stride2 = 0);

struct SubWgradPlan { int ns, cps, nchunks; int grid[3]; int64_t slab_bytes; };      // conv_wgrad_subpixel.hip (GMK_K_CONV_WGRAD_SUBPIXEL)
int gmk_wgrad_subpixel_plan(int B, int H, int W, int cin, int cout, int dy_cstride, int cu_limit, SubWgradPlan* plan);

// conv1x1_stream.hip: the skip convolution's pair of outputs (GMK_K_CONV1X1_PAIR_STREAM) and its weight gradient (GMK_K_CONV1X1_WGRAD_STREAM) at the train step's sizes
int gmk_conv1x1_pair_stream_try(const void* src, int64_t npix, const void* w_rows256, void* out_a, void* out_b, int dtype, void* stream);      // 1 if launched
int gmk_conv1x1_wgrad_stream_try(const void* dy, int dy_cstride, const void* src0, const void* src1, int64_t npix, float* slab, int64_t slab_bytes,
                                 bool x_f16, void* stream);        // > 0 = slabs written

// ---- the stem / head kernels (smallconv.hip) ------------------------------------------------------------------------------------------------
// One launch of the six entry points: the kernel id, its geometry, and the scalars that kernel takes (the others stay 0).  cs: image channels.
struct SmallPlan {
    int kernel, launches;              // launches: cs for the VALU weight gradient (one per image channel), else 1
    unsigned grid, block, lds;
    int ppb, tps, band, nbands, rows;  // rows: the weight gradients' partial rows (= grid = gmk_stem_wgrad_blocks / gmk_head_wgrad_blocks)
    unsigned nblocks, ntiles, ppw;
};
// variant: GMK_DEV_VARIANT (41 keeps the VALU kernels, 42 the exact-fp32 chains); each returns 0 for a shape the entry points refuse
int gmk_expand_plan(int B, int cs, int H, int W, int C, int dtype, int variant, int cu_limit, SmallPlan* p);      // gmk_stem_fwd, gmk_head_dgrad
int gmk_wgrad3_plan(int B, int cs, int H, int W, int C, int dtype, int variant, int cu_limit, SmallPlan* p);      // gmk_stem_wgrad, gmk_head_wgrad
// gmk_head_fwd (stem_dgrad = false), gmk_stem_dgrad: the kernel ids differ.  band < 1 (kernel 0): the image is too wide for the VALU kernel's LDS
int gmk_head_plan(int B, int cs, int H, int W, int C, int dtype, int variant, int cu_limit, bool stem_dgrad, SmallPlan* p);
