// Internal host-side launcher declarations (C++). The public C ABI is include/dtc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include "common.h"

struct dtc_eval_record;  // include/dtc.h

namespace dtc {

// ------------------------------------------------------------------ tuning options (atomic ints)
// X(ID, name, default): the live options only. Variants that measured negative or neutral were
// deleted with their code paths (round 4; their numbers are in DESIGN.md).
#define DTC_OPTION_LIST(X)                                                                                   \
  X(XCD_REMAP, xcd_remap, 1)            /* igemm: tiles sharing operands on one XCD */                       \
  X(DGRAD_CLASSES, dgrad_classes, 1)    /* stride-2 dgrad as output-parity classes */                        \
  X(WGRAD_FAST, wgrad_fast, 1)          /* igemm WGRAD fast loader */                                         \
  X(GRAPHS, graphs, 4)                  /* 0 eager, 1 fwd + bwd hipGraphs, 2 fwd only, 3 bwd only, 4 auto */ \
  X(WGRAD_HALO, wgrad_halo, 224)        /* target workgroups of the halo WGRAD kernel (0 = igemm only) */   \
  X(HALO_CONV, halo_conv, 1)            /* halo FWD/DGRAD for 3x3 s1: 0 off, 1 auto, 2+k force cfg k */     \
  X(HALO_SPLIT, halo_split, 0)          /* halo FWD/DGRAD split-K: 0 auto, k forced */                        \
  X(BWD_STREAMS, bwd_streams, 1)        /* weight gradients on a side stream beside the dgrad/BN chain */    \
  X(CONV_C64, conv_c64, 1)              /* persistent 64->64 3x3 conv for layer1: 1 >= a tile per workgroup, 2 always */           \
  X(BN_FUSED_FIN, bn_fused_fin, 1)      /* BN coefficients folded into the apply kernels */                   \
  X(WGRAD_BATCH, wgrad_batch, 4)        /* up to this many 3x3 s1 wgrads of a bucket per launch */            \
  X(BN_MASK, bn_mask, 1)                /* ReLU mask bits from the forward drive the BN backward */          \
  X(BARRIER_SPIN, barrier_spin, 1)      /* dtc_barrier: 1 poll the event, 0 hipEventSynchronize */           \
  X(STEM_DIRECT, stem_direct, 1)        /* (plan time) direct stem conv, 0 = im2col + GEMM */                 \
  X(WGRAD_XCD, wgrad_xcd, 1)            /* wgrad_halo: tiles of one (problem, split) on one XCD */           \
  X(WGRAD_DIRECT, wgrad_direct, 1)      /* wgrad_halo: a one-split launch writes the scaled dw itself */     \
  X(IGEMM_TILE, igemm_tile, 0)          /* igemm tile: 0 auto, 1 64x64, 2 128x128, 3 64x256 (tuning) */     \
  X(IGEMM_SPLIT, igemm_split, 0)        /* igemm split-K: 0 auto, k forced (tuning) */                        \
  X(DGRAD_CLASS_ORDER, dgrad_class_order, 1) /* stride-2 dgrad classes heaviest first */                      \
  X(STEM_PROLOGUE, stem_prologue, 1)    /* input copy + BN slot zeroing in one launch */                      \
  X(SC_COMPACT, sc_compact, 1)          /* shortcut dx at the stride-2 grid, added by conv1's dgrad */        \
  X(STEM_BN_FUSE, stem_bn_fuse, 1)      /* stem BN backward apply inside the stem weight gradient */          \
  X(BN_RED_ELEMS, bn_red_elems, 16384)  /* bn_bwd_reduce: target elements per workgroup (tuning) */           \
  X(BN_RED_BLOCKS, bn_red_blocks, 256)  /* ... while keeping at least this many workgroups (tuning) */        \
  X(BN_FA_BLOCKS, bn_fa_blocks, 1024)   /* BN fin_apply: target workgroups per launch (tuning) */             \
  X(FORK_LAZY, fork_lazy, 1)            /* fork the wgrad stream only where a wgrad launches */               \
  X(SIDE_PRIO, side_prio, 1)            /* (side stream creation) weight-gradient stream at low priority */  \
  X(SC_FUSE, sc_fuse, 1)                /* projection shortcut inside conv1's forward: 1 layer4, 2/3 wider */ \
  X(STEM_WLDS, stem_wlds, 1)            /* stem forward weight staged in LDS */                               \
  X(HALO_S2, halo_s2, 1)                /* stride-2 3x3 FWD on the column-split halo kernel */                \
  X(WGRAD_S2, wgrad_s2, 1)              /* stride-2 wgrad (+ shortcut) on the halo kernel: 0 off, 1 all, 2 GEN */ \
  X(WGRAD_S2_WGS, wgrad_s2_wgs, 128)    /* stride-2 halo wgrad: target workgroups (split-K slab = wgs x tile) */ \
  X(C64_WGS, c64_wgs, 256)              /* conv_c64 (layer1) persistent grid size */                          \
  X(WGRAD_HALO_L1, wgrad_halo_l1, 0)    /* wgrad_halo target for the one-tile (layer1) geometry (0: wgrad_halo) */ \
  X(DGRAD_SCF, dgrad_scf, 1)            /* shortcut dgrad fused into conv1's parity-class dgrad */            \
  X(BN_CG, bn_cg, 1)                    /* small BN backward as one launch (bn_bwd_cg) ...                  */ \
  X(BN_CG_ELEMS, bn_cg_elems, 262144)   /* ... for tensors of at most this many elements                    */ \
  X(HEAD_FUSED, head_fused, 1)          /* head backward in one launch: 1 always, 2 at <= 64 images */       \
  X(XENT_FUSE, xent_fuse, 1)            /* CrossEntropyLoss backward inside the head backward kernel */     \
  X(COMM_ON_SIDE, comm_on_side, 1)      /* bucket all-reduces on the weight-gradient stream (no comm stream) */ \
  X(BUCKET_TAIL, bucket_tail, 1)        /* (plan time) close the open bucket (>= 1 MB) after layer2.0 */      \
  X(WGRAD_GEN, wgrad_gen, 1)            /* wgrad_halo general step geometry (224x224 model) */                \
  X(WGRAD_TRIM, wgrad_trim, 1)          /* wgrad_halo: no zero-fill DMA for last-round rows past the halo */  \
  X(HALO_GEN, halo_gen, 1)              /* conv_halo general tile geometry (224x224 model) */                 \
  X(BN_RED_UNROLL, bn_red_unroll, 4)    /* bn_bwd_reduce: rows per thread whose loads go together */          \
  X(C64_GEN, c64_gen, 1)                /* conv_c64 general tiles (224x224 layer1) */                         \
  X(SPLITK_INK, splitk_ink, 1)          /* conv split-K summed by the last workgroup per tile (no reduce launch) */ \
  X(COMM_PRIO, comm_prio, 0)            /* (communicator creation) its own stream: 0 normal, 1 most urgent */ \
  X(COMM_TAIL_INLINE, comm_tail_inline, 1) /* the last bucket's all-reduce on the compute stream (no fork / join) */ \
  X(DGRAD_S2H, dgrad_s2h, 1)            /* stride-2 3x3 dgrad (+ shortcut) as a halo sub-pixel conv: 1 K <= 256, 2 all */ \
  X(HALO_SMALL, halo_small, 1)          /* halo FWD/DGRAD: 64x64 double-buffered tiles where they give <= 512 workgroups */

enum {
#define DTC_OPT_ENUM(id, name, def) OPT_##id,
  DTC_OPTION_LIST(DTC_OPT_ENUM)
#undef DTC_OPT_ENUM
  OPT_COUNT
};
int option_get(int id);
int option_set(const char* name, int value);
int option_epoch();  // bumped by every option_set (captured graphs bake the options in)

// ------------------------------------------------------------------ convolution
struct ConvShape {
  int N, H, W, C;  // input NHWC
  int K, R, S;     // filters KRSC
  int stride, pad;
};
enum { CONV_FWD = 0, CONV_DGRAD = 1, CONV_WGRAD = 2 };
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- each kernel family's own planner (which family a conv runs on is conv_route's question)
// Implicit GEMM (igemm.hip), every geometry: tile (64x64 / 64x256 / 128x128), split-K factor and reduction steps;
// cls: a stride-2 DGRAD as four output-parity-class GEMMs in one launch (even H and W; no split-K)
struct GemmPlan {
  int bm, bn, splits, num_kt;
  size_t slab_bytes;  // fp32 slab of `splits` partial outputs (FWD / DGRAD: 0 with one split)
};
bool dgrad_class_mode(const ConvShape& s);  // option dgrad_classes and the geometry
GemmPlan igemm_plan(const ConvShape& s, int pass, bool cls);
bool conv_c64_ok(const ConvShape& s);  // persistent 64-channel 3x3 stride-1 FWD / DGRAD (conv_c64.hip)
// Halo-tiled 3x3 FWD / DGRAD, stride 1, and FWD stride 2 column-split (conv_halo.hip): configuration for the pass
// (cfg -1: not applicable) and its split-K factor over the reduction chunks
struct HaloPlan {
  int cfg, split;
  int gen = 0;  // 1: general tile geometry (rows of seg columns, 64-bit tile bases; conv_halo.hip)
};
HaloPlan conv_halo_plan(const ConvShape& s, int pass);
size_t conv_halo_slab_bytes(const ConvShape& s, int pass, const HaloPlan& hp);  // fp32 split-K slab of the plan
// (the slab a conv_halo launch writes is conv_halo_slab_bytes of the plan it is given: split 1 writes none)
size_t igemm_slab_used(const ConvShape& s, int pass, const GemmPlan& pl);  // fp32 slab an igemm launch of pl writes
bool dgrad_s2_halo_ok(const ConvShape& s);  // stride-2 3x3 DGRAD as a halo-tiled sub-pixel conv (dgrad_s2.hip)
// Halo-tiled 3x3 WGRAD (wgrad_halo.hip): the split count it would use (0: not applicable / disabled) for stride 1,
// nprob (<= DTC_WG_BATCH) problems per launch, and for stride 2 (conv1 of a projection block, + its shortcut).
constexpr int DTC_WG_BATCH = 4;
int wgrad_halo_splits(const ConvShape& s, int nprob = 1);
int wgrad_s2_splits(const ConvShape& s);
size_t conv_wgrad_s2_slab_bytes(const ConvShape& s, int splits);  // 9 taps + the shortcut's [K][C] per split
// fp32 slab the launches write when asked for `splits` (no split is empty, so fewer may run; 0: one split that
// writes dw itself, option wgrad_direct)
size_t conv_wgrad_halo_slab_used(const ConvShape& s, int nprob, int splits, bool dw_given);
size_t conv_wgrad_s2_slab_used(const ConvShape& s, int splits);

// ---- the router (conv_route.cpp): the one place that knows the families' order of precedence
enum ConvKernel {  // GEMM_CLASSES: igemm's stride-2 DGRAD parity classes (take a compact residual / the fused shortcut)
  CONV_K_GEMM, CONV_K_GEMM_CLASSES, CONV_K_C64, CONV_K_HALO, CONV_K_DGRAD_S2, CONV_K_WGRAD_HALO, CONV_K_WGRAD_S2
};
struct ConvRequest {  // what a launch branches on besides the shape
  bool res = false;  // DGRAD: a residual is added
  bool sc = false;   // the block's 1x1 stride-2 shortcut in the same launch (conv_fwd_sc / conv_dgrad_sc)
  int dw_cols = 0, dw_ld = 0;  // WGRAD: a partial dw (0: whole rows)
  int nprob = 1;               // WGRAD: problems per launch (conv_wgrad_batch)
  bool batch = false;          // WGRAD: conv_wgrad_batch's contract (the halo kernel or an error); conv_launch only
  size_t slab_bytes = SIZE_MAX;  // fp32 slab on hand (default: sizing -- whatever the route wants)
};
struct ConvRoute {
  int kernel = CONV_K_GEMM;
  GemmPlan gemm{};          // GEMM kernels: splits final for the slab on hand
  HaloPlan halo{-1, 1};     // CONV_K_HALO: split 1 when the slab on hand is too small
  int splits = 0;           // CONV_K_WGRAD_HALO / _S2
  bool dw_whole = true;     // WGRAD: dw is written in whole rows (the halo kernels may write it themselves)
  size_t slab_bytes = 0;    // fp32 slab the pass wants (0 = none): this route's and its GEMM fallback's
  bool sc_ok = false;       // 3x3 stride 2: the pass has a shortcut-fused launch (with req.sc: this route is it)
};
ConvRoute conv_route(const ConvShape& s, int pass, const ConvRequest& req = ConvRequest{});
// What a launcher below does with a request: conv_route's answer for the slab on hand (req.sc: the shortcut-fused
// launcher of the pass, which takes no slab for FWD / DGRAD), the fp32 slab bytes that launch writes, and why the
// launcher returns an error instead (nullptr: it launches). The launchers and dtc_conv2d_route_query both ask here.
struct ConvLaunch {
  ConvRoute route;
  size_t slab_used = 0;
  const char* refused = nullptr;
};
ConvLaunch conv_launch(const ConvShape& s, int pass, const ConvRequest& req);

// ---- launchers (conv_route.cpp): route, then the family's launch
// y = conv(x, w) (bf16 NHWC out); optional BN statistics of the bf16 output into
// stats (sum, sum of squares; exact fixed-point accumulators, DTC_STAT_WORDS(K) int64: common.h).
// `ts` (optional, every conv launcher): a DTC_PROF_SLOT_U64 slot receiving the entry times of the
// first workgroups and every workgroup's exit time in s_memrealtime ticks (graph-safe per-call timing).
// tick (optional): >= DTC_TICKS zeroed u32 arrival counters reserved for the launch stream (the executor's
// workspace: one set per stream); with it a split-K conv reduces its slab inside the kernel (the last
// workgroup of each output tile), else a separate reduction launch does. The counters are left zero.
#define DTC_TICKS 8192
int conv_fwd(const ConvShape& s, const u16* x, const u16* w, u16* y, int64_t* stats, float* slab,
             size_t slab_bytes, hipStream_t st, u64* ts = nullptr, unsigned* tick = nullptr);
// 3x3 stride-2 conv and the 1x1 stride-2 projection shortcut of the same input in one launch
bool conv_fwd_sc_ok(const ConvShape& s, const ConvShape& sc);
int conv_fwd_sc(const ConvShape& s, const ConvShape& sc, const u16* x, const u16* w, u16* y, int64_t* stats,
                const u16* wsc, u16* ysc, int64_t* stats_sc, hipStream_t st, u64* ts = nullptr);
// dx = conv_transpose(dy, w) (+ res), bf16 NHWC.
// dx may alias res (in place: each element is read and written by the same lane).
// res_compact: res is [N][H/2][W/2][C] (a 1x1 stride-2 shortcut's dx at its only nonzero parity),
// added at the (even, even) pixels only -- needs the parity-class route (CONV_K_GEMM_CLASSES).
int conv_dgrad(const ConvShape& s, const u16* dy, const u16* w, u16* dx, const u16* res, float* slab,
               size_t slab_bytes, hipStream_t st, u64* ts = nullptr, int res_compact = 0, unsigned* tick = nullptr);
// dx = dgrad(dy, w) + dgrad_1x1_s2(dsc, wsc) for a projection block's 3x3 stride-2 conv1 and its shortcut
// in one launch (dsc [N][H/2][W/2][K], wsc [K][C]); needs sc_ok of the DGRAD route of s
int conv_dgrad_sc(const ConvShape& s, const u16* dy, const u16* w, u16* dx, const u16* dsc, const u16* wsc,
                  hipStream_t st, u64* ts = nullptr);
// dw[k][0:dw_cols] (row stride dw_ld) = scale * sum_pixels dy (x) im2col(x); fp32
int conv_wgrad(const ConvShape& s, const u16* x, const u16* dy, float* dw, int dw_cols, int dw_ld, float scale,
               float* slab, size_t slab_bytes, hipStream_t st, u64* ts = nullptr);
// dw and the block's 1x1 stride-2 shortcut's dw_sc [K][C] (from dsc) in one conv_wgrad_s2 launch; DTC_EINVAL without
// the stride-2 halo route or with a slab smaller than the splits that run need
int conv_wgrad_sc(const ConvShape& s, const u16* x, const u16* dy, const u16* dsc, float* dw, float* dw_sc, float scale,
                  float* slab, size_t slab_bytes, hipStream_t st, u64* ts = nullptr);
// nprob (<= DTC_WG_BATCH) weight gradients of one 3x3 stride-1 geometry in one halo launch + one reduce launch: dw[i] =
// scale * wgrad(x[i], dy[i]). DTC_EINVAL when there is no halo plan or the slab is too small (then: one by one).
int conv_wgrad_batch(const ConvShape& s, int nprob, const u16* const* x, const u16* const* dy, float* const* dw,
                     float scale, float* slab, size_t slab_bytes, hipStream_t st, u64* ts = nullptr);

// ---- the families' launches (called with the router's plan)
// igemm.hip. FWD: wsc != null also computes the shortcut (ysc, stats_sc; one split). DGRAD: cls as planned; with cls,
// res_compact or the fused shortcut (dsc, wsc). Split-K is reduced by splitk_reduce; WGRAD only writes its slab.
int igemm_fwd(const ConvShape& s, const GemmPlan& pl, const u16* x, const u16* w, u16* y, int64_t* stats, float* slab,
              const u16* wsc, u16* ysc, int64_t* stats_sc, hipStream_t st, u64* ts);
int igemm_dgrad(const ConvShape& s, const GemmPlan& pl, bool cls, const u16* dy, const u16* w, u16* dx, const u16* res,
                int res_compact, const u16* dsc, const u16* wsc, float* slab, hipStream_t st, u64* ts);
int igemm_wgrad(const ConvShape& s, const GemmPlan& pl, const u16* x, const u16* dy, float* slab, hipStream_t st,
                u64* ts);
int conv_c64(const ConvShape& s, int mode, const u16* src, const u16* w, u16* out, const u16* res, int64_t* stats,
             hipStream_t st, u64* ts);
// FWD: stats optional, wsc / out2 / stats2 the fused shortcut (stride 2); DGRAD: res optional
int conv_halo(const ConvShape& s, int mode, const HaloPlan& hp, const u16* src, const u16* w, u16* out,
              const u16* res, int64_t* stats, float* slab, hipStream_t st, u64* ts = nullptr,
              const u16* wsc = nullptr, u16* out2 = nullptr, int64_t* stats2 = nullptr, unsigned* tick = nullptr);
// optionally + the 1x1 stride-2 shortcut's dgrad (dsc [N][H/2][W/2][K], wsc [K][C]) at the even / even pixels
int conv_dgrad_s2_halo(const ConvShape& s, const u16* dy, const u16* w, u16* dx, const u16* dsc, const u16* wsc,
                       hipStream_t st, u64* ts = nullptr);
// writes slab[nprob][used][K][9C] (reduce separately); dw (optional): when the launch uses ONE split its epilogue
// writes dw[i] = scale * sum directly (no slab, no reduce; *used_splits = 0 tells the caller)
int conv_wgrad_halo(const ConvShape& s, int nprob, const u16* const* x, const u16* const* dy, float* slab, int splits,
                    int* used_splits, hipStream_t st, u64* ts, float* const* dw = nullptr, float scale = 1.f);
// 3x3 stride-2 weight gradient on the column-split halo kernel, with dsc != null also the block's 1x1 stride-2
// shortcut's (dw_sc[k][c]); split-K (wgrad_s2_splits) over output pixels into slab ([splits][K][9C | C]) + reduces.
int conv_wgrad_s2(const ConvShape& s, int splits, const u16* x, const u16* dy, const u16* dsc, float* dw, float* dw_sc,
                  float scale, float* slab, size_t slab_bytes, hipStream_t st, u64* ts = nullptr);
// out = bf16(sum_s slab[s] (+ res)) (+ the BN statistics of out): the separate split-K reduction
int splitk_reduce(const float* slab, int splits, int M, int Nc, u16* out, const u16* res, int64_t* stats,
                  hipStream_t st, u64* ts = nullptr);
// dw[i][k][0:ncols] (row stride ldo) = scale * sum_s slab[i][s][k][0:RSC], i < nprob (igemm.hip's deterministic
// reduce); _pair: two dense problems of row lengths ld0 >= ld1
int wgrad_reduce_to(const float* slab, int splits, int K, int RSC, int ncols, int ldo, float scale, float* const* dw,
                    int nprob, hipStream_t st, u64* ts = nullptr);
int wgrad_reduce_pair(const float* slab, int splits, int K, int ld0, float* dw0, size_t stride, int ld1, float* dw1,
                      float scale, hipStream_t st, u64* ts = nullptr);
// per slot i of ts[n][DTC_PROF_SLOT_U64]: acc[i] += (max end - min start, 1) if stamped; cells reset
int prof_accumulate(u64* ts, int n, u64* acc, hipStream_t st);

// fp32 mode (conv_f32.hip): fp32 in / fp32 out implicit GEMM on v_mfma_f32_16x16x4_f32.
// FWD: out = y (+ BN stats into `stats`); DGRAD: out = dx (+ res); WGRAD: dw[k][0:dw_cols] (row stride
// dw_ld; 0 = R*S*C) = scale * sum over pixels, via split-K slabs in `slab`. C and K multiples of 16.
int conv_f32(const ConvShape& s, int mode, const float* a, const float* b, float* out, const float* res,
             int64_t* stats, float* dw, int dw_cols, int dw_ld, float scale, float* slab, size_t slab_bytes,
             hipStream_t st, u64* ts = nullptr);
size_t f32_conv_workspace(const ConvShape& s, int mode);  // fp32 slab bytes the pass wants
int f32_stem_im2col(const float* x, float* cols, int N, int H, int W, hipStream_t st);  // [N*H*W][32]
int f32_stem_pack_weight(const float* w27, float* w32, int K, hipStream_t st);          // [K][27] -> [K][32]

// ------------------------------------------------------------------ batch norm (NHWC, C channels, M pixels)
// forward finalize: mean/invstd/scale/shift from stats; running-stat update; stats re-zeroed.
int bn_fwd_finalize(int64_t* stats, int C, int64_t count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches, float momentum, float eps,
                    float* mean, float* invstd, float* scale, float* shift, hipStream_t st);
// eval mode: scale/shift from running statistics (mean/invstd also written for reference)
int bn_eval_coef(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                 float eps, float* mean, float* invstd, float* scale, float* shift, hipStream_t st);
// the same for every BatchNorm of a network in ONE launch, driven by a by-value descriptor table (the kernel
// argument segment holds it: nothing is allocated). Per channel the arithmetic is bn_eval_coef's own device
// function (bn_coef.h). blk0 is filled by the launcher.
constexpr int DTC_EVAL_BN_MAX = 20;  // ResNet-18: 20 BatchNorms, 72 B each = 1.4 KB of kernel arguments
struct BnEvalEntry {
  int C = 0, blk0 = 0;  // channels; first workgroup of this BN (256 channels per workgroup)
  const float* gamma = nullptr;
  const float* beta = nullptr;
  const float* rmean = nullptr;
  const float* rvar = nullptr;
  float* mean = nullptr;
  float* invstd = nullptr;
  float* scale = nullptr;
  float* shift = nullptr;
};
struct BnEvalTable {
  BnEvalEntry e[DTC_EVAL_BN_MAX];
  int n = 0;
};
int bn_eval_coef_all(BnEvalTable& tab, float eps, hipStream_t st);
// y = relu(x*scale + shift)
int bn_apply_relu(const u16* x, const float* scale, const float* shift, u16* y, int64_t M, int C, hipStream_t st);
// y = relu(x*scale + shift + res)            (identity shortcut)
int bn_apply_add_relu(const u16* x, const float* scale, const float* shift, const u16* res, u16* y, int64_t M,
                      int C, hipStream_t st);
// y = relu(x*scale + shift + x2*scale2 + shift2)   (projection shortcut: two BNs)
int bn_apply_dual_relu(const u16* x, const float* scale, const float* shift, const u16* x2, const float* scale2,
                       const float* shift2, u16* y, int64_t M, int C, hipStream_t st);
// y = x*scale + shift (no activation; eval helpers / tests)
int bn_apply(const u16* x, const float* scale, const float* shift, u16* y, int64_t M, int C, hipStream_t st);
// fp32-activation versions of the four (fp32 mode: the reference without --amp)
int bn_apply_relu(const float* x, const float* scale, const float* shift, float* y, int64_t M, int C, hipStream_t st);
int bn_apply_add_relu(const float* x, const float* scale, const float* shift, const float* res, float* y, int64_t M,
                      int C, hipStream_t st);
int bn_apply_dual_relu(const float* x, const float* scale, const float* shift, const float* x2, const float* scale2,
                       const float* shift2, float* y, int64_t M, int C, hipStream_t st);
int bn_apply(const float* x, const float* scale, const float* shift, float* y, int64_t M, int C, hipStream_t st);

// Fused finalize + apply: the coefficients are computed by the consumer from the statistic slots
// (bn.hip); the first pixel block writes the saved / running statistics (forward) or dgamma /
// dbeta (backward). The slots must be zeroed before their producers run (executor: memset node).
struct BnFwdArgs {
  const int64_t* stats = nullptr;  // DTC_STAT_WORDS(C): sum, sum of squares of the bf16 conv output
  int64_t count = 0;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  float* rmean = nullptr;
  float* rvar = nullptr;
  int64_t* nbt = nullptr;
  float momentum = 0.1f, eps = 1e-5f;
  float* mean = nullptr;    // saved for backward
  float* invstd = nullptr;
};
struct BnBwdArgs {
  const int64_t* acc = nullptr;  // [SLOTS][2][C] sum(dz), sum(dz*xhat)
  int64_t count = 0;
  const float* gamma = nullptr;
  const float* mean = nullptr;
  const float* invstd = nullptr;
  float gscale = 1.f;
  float* dgamma = nullptr;
  float* dbeta = nullptr;
};
// mode: 1 relu, 2 add residual x2 + relu, 3 dual BN (x2 normalised by a2) + relu
// mask (optional): ReLU mask bits of y (byte o/8 for element offset o) for the mask-bit backward
int bn_fin_apply(int mode, const u16* x, const BnFwdArgs& a1, const u16* x2, const BnFwdArgs* a2, u16* y, int64_t M,
                 int C, hipStream_t st, uint8_t* mask = nullptr, u64* ts = nullptr);
// Mask-bit BN backward (the executor's default): dz = dy * mask bit is formed where it is used, never
// stored by the reduction. Reduce: sums only (dy, bits, x read: 4.125 B/element); apply: dx (and
// dzo = dz if non-null, may alias dy) from dy, bits, x. bn_mask_apply: dz alone (parity captures).
int bn_bwd_reduce_mask(const u16* dy, const uint8_t* mbits, const u16* x1, const float* mean1, const float* invstd1,
                       int64_t* acc1, const u16* x2, const float* mean2, const float* invstd2, int64_t* acc2, int64_t M,
                       int C, hipStream_t st, u64* ts = nullptr);
int bn_bwd_fin_apply_mask(const u16* dy, const uint8_t* mbits, u16* dzo, const u16* x1, const BnBwdArgs& a1, u16* dx1,
                          const u16* x2, const BnBwdArgs* a2, u16* dx2, int64_t M, int C, hipStream_t st,
                          u64* ts = nullptr);
int bn_mask_apply(const u16* dy, const uint8_t* mbits, u16* dz, int64_t M, int C, hipStream_t st);
// One-launch mask-bit BN backward of a small tensor (bn_bwd_cg_ok: M <= 4096 pixels, 2048 dual): reduce +
// coefficients + apply (dz, dx1 [, dx2], dgamma / dbeta x gscale) in one workgroup per 8 channels; the
// statistic slots are unused
bool bn_bwd_cg_ok(int64_t M, int C, bool dual);
int bn_bwd_cg(const u16* dy, const uint8_t* mbits, u16* dzo, const u16* x1, const BnBwdArgs& a1, u16* dx1,
              const u16* x2, const BnBwdArgs* a2, u16* dx2, int64_t M, int C, hipStream_t st, u64* ts = nullptr);
int bn_bwd_fin_apply(const u16* dz, const u16* x1, const BnBwdArgs& a1, u16* dx1, const u16* x2, const BnBwdArgs* a2,
                     u16* dx2, int64_t M, int C, hipStream_t st);
int bn_fin_apply(int mode, const float* x, const BnFwdArgs& a1, const float* x2, const BnFwdArgs* a2, float* y,
                 int64_t M, int C, hipStream_t st);
int bn_bwd_fin_apply(const float* dz, const float* x1, const BnBwdArgs& a1, float* dx1, const float* x2,
                     const BnBwdArgs* a2, float* dx2, int64_t M, int C, hipStream_t st);

// slot 0 <- the exact sum over the slots (lo carried into hi), the others zeroed (SyncBN's collective)
int bn_fold_slots(int64_t* slots, int C, hipStream_t st);
// The arguments of a BN-backward reduction as one bundle: dy is the gradient of a post-ReLU BN output
// y = relu(bn(x1) [+ bn(x2)]) (reference src/*/net.py:41-44, 108); the passes below accumulate sum(dz) and
// sum(dz * xhat) of dz = dy * [y > 0]. Behind a data gradient they run in place on the conv_dgrad's dx.
struct BnbArgs {
  const u16* ym = nullptr;      // post-ReLU activation y (mask source), or ...
  const uint8_t* mb = nullptr;  // ... the forward's ReLU mask bits of y (bit e & 7 of byte e >> 3 for element e)
  const u16* x1 = nullptr;      // input of the (first) BN: the conv output it normalised
  const float *mean1 = nullptr, *invstd1 = nullptr;
  int64_t* acc1 = nullptr;      // [SLOTS][2][C]: sum dz, sum dz * xhat
  const u16* x2 = nullptr;      // second BN sharing dz (projection shortcut) or null
  const float *mean2 = nullptr, *invstd2 = nullptr;
  int64_t* acc2 = nullptr;
};
// backward: dz = dy * [y > 0] (mask optional); accumulates sum(dz), sum(dz*xhat1) [, sum(dz*xhat2)]
int bn_bwd_reduce(const u16* dy, const u16* ymask, const u16* x1, const float* mean1, const float* invstd1,
                  int64_t* acc1, const u16* x2, const float* mean2, const float* invstd2, int64_t* acc2, u16* dz,
                  int64_t M, int C, hipStream_t st);
int bn_bwd_reduce(const float* dy, const float* ymask, const float* x1, const float* mean1, const float* invstd1,
                  int64_t* acc1, const float* x2, const float* mean2, const float* invstd2, int64_t* acc2, float* dz,
                  int64_t M, int C, hipStream_t st);
// dgamma/dbeta (scaled by gscale) into the flat grad buffer; apply coefficients coef[3][C]; acc re-zeroed.
int bn_bwd_finalize(int64_t* acc, int C, int64_t count, const float* gamma, const float* mean,
                    const float* invstd, float gscale, float* dgamma, float* dbeta, float* coef, hipStream_t st);
// dx1 = A1*dz + B1*x1 + C1 [; dx2 = A2*dz + B2*x2 + C2]
int bn_bwd_apply(const u16* dz, const u16* x1, const float* coef1, u16* dx1, const u16* x2, const float* coef2,
                 u16* dx2, int64_t M, int C, hipStream_t st);
int bn_bwd_apply(const float* dz, const float* x1, const float* coef1, float* dx1, const float* x2, const float* coef2,
                 float* dx2, int64_t M, int C, hipStream_t st);

// ------------------------------------------------------------------ stem / head / loss
// x fp32 NCHW [N][3][H][W] -> im2col bf16 [N*H*W][64] (3x3 pad 1 taps, (r,s,c) order, zero padded)
int stem_im2col(const float* x, u16* cols, int N, int H, int W, hipStream_t st);
// w bf16 [64][27] -> [64][64] zero padded
int stem_pack_weight(const u16* w27, u16* w64, int K, hipStream_t st);
// Direct stem conv (stem.hip): im2col gathered into LDS per 256-pixel tile, one K=32 MFMA k-step.
// fwd: y [N*H*W][64] bf16 (+ BN statistics of the bf16 output into stats[SLOTS][2][64] if non-null)
// from fp32 NCHW x and the bf16 [64][27] weight; wgrad: dw27 [64][27] fp32 = scale * sum.
int stem_fwd(const float* x, const u16* w27, u16* y, int64_t* stats, int N, int H, int W, hipStream_t st,
             u64* ts = nullptr);
size_t stem_wgrad_slab_bytes(int64_t M);
int stem_wgrad(const float* x, const u16* dy, float* dw27, float scale, int N, int H, int W, float* slab,
               size_t slab_bytes, hipStream_t st, u64* ts = nullptr);
// stem weight gradient with the stem BN's backward apply fused: dc = A*(dy*bit) + B*c + Cc formed per
// tile in LDS from (dy, mask bits, the conv output c) and the BN's slots (a: as bn_bwd_fin_apply's)
int stem_wgrad_bn(const float* x, const u16* dy, const uint8_t* mbits, const u16* c, const BnBwdArgs& a, float* dw27,
                  float scale, int N, int H, int W, float* slab, size_t slab_bytes, hipStream_t st, u64* ts = nullptr);
// feat[n][c] = bf16round(mean_hw act); logits[n][j] = feat . W[j] + b[j]
int head_fwd(const u16* act, int N, int HW, int C, const u16* wfc, const float* bfc, int ncls, float* feat,
             float* logits, hipStream_t st);
// mean cross entropy; lse per row
// the same plus loss * (*scale) into `scaled` and the loss into the host word `host` (optional), one launch
int xent_fwd_fused(const float* logits, const int64_t* labels, int N, int ncls, float* loss, float* lse,
                   const float* scale, float* scaled, float* host, hipStream_t st);
int xent_fwd(const float* logits, const int64_t* labels, int N, int ncls, float* loss, float* lse,
             hipStream_t st);
// evaluation metrics of one batch (metrics.hip): mean cross-entropy (bit-identical to xent_fwd's), the row count
// and the top-1 / top-k hit counts into one 16-byte device record, one launch (N <= 4096)
int eval_metrics(const float* logits, const int64_t* labels, int N, int ncls, int topk, ::dtc_eval_record* rec,
                 hipStream_t st);
// dlogits = (softmax - onehot) * (*gscale) / N
int xent_bwd(const float* logits, const int64_t* labels, const float* lse, const float* gscale, int N, int ncls,
             float* dlogits, hipStream_t st);
// Soft targets q = (1 - smoothing) * (lam * onehot(labels_a) + (1 - lam) * onehot(labels_b)) + smoothing / ncls
// per row (label smoothing, Mixup, CutMix); labels_b == lam == nullptr: lam = 1. The forward is xent_fwd_fused
// with the same lse bits; with smoothing = 0 and no labels_b loss and dlogits are the hard kernels' bit for bit.
int xent_soft_fwd_fused(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                        float smoothing, int N, int ncls, float* loss, float* lse, const float* scale, float* scaled,
                        float* host, hipStream_t st);
// the same loss without the row cap, two launches (xent_fwd's form): the fallback for N > 4096
int xent_soft_fwd(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                  float smoothing, int N, int ncls, float* loss, float* lse, hipStream_t st);
int xent_soft_bwd(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                  float smoothing, const float* lse, const float* gscale, int N, int ncls, float* dlogits,
                  hipStream_t st);
// dW = scale*dlogits^T feat ; db = scale*sum dlogits ; dact[n][hw][c] = (dlogits . W)[c] / HW
size_t head_bwd_workspace(int N, int C, int ncls);
// fp32 mode: fp32 activations and fp32 Linear weights, no autocast rounding
int head_fwd(const float* act, int N, int HW, int C, const float* wfc, const float* bfc, int ncls, float* feat,
             float* logits, hipStream_t st);
// xa != nullptr: the CrossEntropyLoss backward is fused in -- dlogits is computed from (logits, labels,
// lse, gscale) exactly as xent_bwd does, used directly, and also stored into `dlogits` (an output then)
// soft: the soft-target gradient (xent_soft_bwd) from labels (= labels_a), labels_b (never null then: labels_a
// when there is no second label), lam (nullptr: 1) and smoothing
struct XentArgs {
  const float* logits = nullptr;
  const int64_t* labels = nullptr;
  const float* lse = nullptr;
  const float* gscale = nullptr;
  const int64_t* labels_b = nullptr;
  const float* lam = nullptr;
  float smoothing = 0.f;
  bool soft = false;
};
int head_bwd(const float* dlogits, const float* feat, const float* wfc, int N, int HW, int C, int ncls, float scale,
             float* dw, float* db, float* dact, float* ws, size_t ws_bytes, hipStream_t st,
             const XentArgs* xa = nullptr);
int head_bwd(const float* dlogits, const float* feat, const u16* wfc, int N, int HW, int C, int ncls, float scale,
             float* dw, float* db, u16* dact, float* ws, size_t ws_bytes, hipStream_t st, const XentArgs* xa = nullptr);

// ------------------------------------------------------------------ optimizer / amp / casts
// Nesterov SGD over a flat buffer (torch.optim.SGD semantics, dampening 0).
int sgd_nesterov(float* p, const float* g, float* mom, u16* p_bf16, int64_t n, float lr, float wd, float mu,
                 const float* inv_scale, const int* found_inf, hipStream_t st);
// Adam / AdamW over a flat buffer (torch.optim.Adam / AdamW semantics, amsgrad off): a one-thread tick that
// advances the device-side step count in `state` (DTC_ADAM_STATE_WORDS zeroed 32-bit words, 16-byte aligned)
// unless *found_inf, then the update. The scalars are doubles: 1-beta, 1-lr*wd and the bias corrections are
// formed in double, as torch forms them from Python floats.
#define DTC_ADAM_STATE_WORDS 4
int adam_flat(float* p, const float* g, float* m, float* v, u16* p_bf16, int64_t n, void* state, double lr,
              double beta1, double beta2, double eps, double wd, int decoupled, const float* inv_scale,
              const int* found_inf, hipStream_t st);
// total_norm = inv_scale * ||g||_2 and grad_mult = inv_scale * min(1, max_norm / (total_norm + 1e-6)), on the
// device; double accumulation in a fixed order (bit-reproducible). workspace: grad_norm_workspace_bytes(n).
size_t grad_norm_workspace_bytes(int64_t n);
int grad_norm_clip(const float* g, int64_t n, const float* inv_scale, double max_norm, void* workspace,
                   float* total_norm, float* grad_mult, hipStream_t st);
// Segment plan (lars.hip): where each parameter tensor lies in the flat buffers. The handle holds host data only
// (the validated table and the chunk -> segment work map); bind uploads both into caller-owned device memory of
// segplan_device_bytes() bytes (tables, one partial slot of two doubles per chunk, per-segment results).
struct SegDesc {  // layout of the ABI's dtc_seg
  int64_t offset, numel;
  int32_t flags, reserved;  // flags bit 0: ADAPT (trust ratio and weight decay apply)
};
struct SegPlan;
int64_t segplan_chunk_elems();
int segplan_create(SegPlan** out, const SegDesc* segs, int nseg);
int segplan_destroy(SegPlan* plan);
int segplan_num_segments(const SegPlan* plan);
size_t segplan_device_bytes(const SegPlan* plan);
int segplan_bind(SegPlan* plan, void* dev, size_t bytes, hipStream_t st);
// seg_out[s] (optional, fp32 [nseg][3]) = (||p_s||, |*gmul| * ||g_s||, ratio_s); double sums in a fixed order. Two
// launches. Here ratio_s is the bare norm ratio ||p_s|| / (|*gmul| ||g_s||) of an ADAPT segment (1 where a norm is
// zero and for the others); lars_flat writes the trust ratio it applied.
int seg_norms(SegPlan* plan, const float* p, const float* g, const float* gmul, float* seg_out, hipStream_t st);
// LARS over the plan's segments: the norm pass, the ratios, the momentum update with the bf16 shadow. Three launches.
int lars_flat(SegPlan* plan, float* p, const float* g, float* mom, u16* p_bf16, double lr, double wd, double mu,
              int nesterov, double trust_coef, double eps, int trust_clip, const float* inv_scale,
              const int* found_inf, float* seg_out, hipStream_t st);
// Weight EMA (ema.hip) over 1..DTC_EMA_MAX_RANGES flat ranges in one update launch behind a one-thread tick:
// ema += (src - ema) * w, ema_bf16 = bf16(ema) where given; `state` is DTC_EMA_STATE_WORDS zeroed 32-bit words
// (16-byte aligned): word 0 the int32 count of updates, word 1 the fp32 w of the last one. Skipped when *found_inf.
#define DTC_EMA_STATE_WORDS 4
#define DTC_EMA_MAX_RANGES 4
struct EmaRange {  // layout of the ABI's dtc_ema_range
  float* ema;
  const float* src;
  u16* ema_bf16;
  int64_t n;
};
int ema_update(const EmaRange* ranges, int nranges, void* state, double decay, int warmup, const int* found_inf,
               hipStream_t st);
// Gradient accumulation (accum.hip) over one fp32 range, mode = the ABI's DTC_ACCUM_STORE / ADD / FINISH: acc = g,
// acc = acc + g, g = g + acc, one rounded fp32 add per element. A workgroup of DTC_ACCUM_THREADS takes chunks of
// DTC_ACCUM_THREADS * DTC_ACCUM_UNROLL float4 rows; the grid is capped at DTC_ACCUM_MAX_BLOCKS. One launch.
#define DTC_ACCUM_THREADS 256
#define DTC_ACCUM_UNROLL 4
#define DTC_ACCUM_MAX_BLOCKS 1024
int grad_accum(float* acc, float* g, int64_t n, int mode, hipStream_t st);
// bf16 gradient compression (compress.hip) over one range: c = bf16_rne(acc ? g + acc : g) (one rounded fp32 add,
// then one rounding) and g = widen(c) (exact). fp32 pointers 16-byte aligned, c 8-byte aligned, n a multiple of 4.
// A workgroup of DTC_COMPRESS_THREADS takes chunks of DTC_COMPRESS_THREADS * DTC_COMPRESS_UNROLL rows of 8 elements
// (decompress: twice as many rows of 4); the grid is capped at DTC_COMPRESS_MAX_BLOCKS. One launch each.
#define DTC_COMPRESS_THREADS 256
#define DTC_COMPRESS_UNROLL 4
#define DTC_COMPRESS_MAX_BLOCKS 1024
int grad_compress_bf16(const float* g, const float* acc, u16* c, int64_t n, hipStream_t st);
int grad_decompress_bf16(const u16* c, float* g, int64_t n, hipStream_t st);
// PowerSGD (powersgd.hip): rank-r gradient compression on the flat gradient buffer. The plan (host data; bind uploads
// its tables into caller-owned device memory that also holds the back-project slots and counters) is built from a
// sorted table of tensors; rank 0 = all-reduced as it is. what of psgd_plan_numel: 0 P, 1 Q, 2 uncompressed,
// 3 staging (= uncompressed + P) elements, 4 the stride between the two Q copies. q: [2][stride] fp32 (q[0] the warm
// start kept across a non-finite step, q[1] the working copy the Q collective runs on); staging: [uncompressed | P];
// state: 4 int32 words, zeroed by the caller (word 0: 1 = the next warm start is q[1]; word 1: the last step was
// non-finite); e (error feedback) may be null. One launch each.
struct PsgdDesc {  // layout of the ABI's dtc_psgd_tensor
  int64_t offset, rows, cols;
  int32_t rank, reserved;
};
struct PsgdPlan;
int psgd_plan_create(PsgdPlan** out, const PsgdDesc* tensors, int n);
int psgd_plan_destroy(PsgdPlan* plan);
int64_t psgd_plan_numel(const PsgdPlan* plan, int what);
size_t psgd_plan_device_bytes(const PsgdPlan* plan);
int psgd_plan_bind(PsgdPlan* plan, void* dev, size_t bytes, hipStream_t st);
int psgd_orthonormalize(PsgdPlan* plan, int what, float* q, float* staging, int* state, double eps, hipStream_t st);
int psgd_project(PsgdPlan* plan, const float* g, const float* e, const float* q, float* staging, hipStream_t st);
int psgd_backproject(PsgdPlan* plan, const float* g, const float* e, const float* staging, float* q, hipStream_t st);
int psgd_reconstruct(PsgdPlan* plan, float* g, float* e, const float* staging, const float* q, int* state, double c,
                     hipStream_t st);
// SAM / ASAM (sam.hip) over the whole flat buffer. perturb: p_saved = p, p += coef * g (adaptive: * p * p) with
// coef = rho * m / (|m| * ||t|| + eps), t = g or p * g, m = *gmul, p_bf16 = bf16(p); a non-finite norm moves nothing
// and marks `state` (DTC_SAM_STATE_WORDS 32-bit words, 16-byte aligned: fp32 coef, fp32 norm, int32 skipped) --
// three launches (norm pass into sam_workspace_bytes(n) of slots, finalize, update). restore: p = p_saved, p_bf16 =
// bf16(p), *found_inf = 1 if the perturb was skipped -- one launch. Up to the ABI's DTC_SAM_MAX_KEEP small ranges
// are copied aside by the perturb and back by the restore as 8-byte words, inside those launches. The update and
// restore kernels take chunks of DTC_SAM_THREADS * DTC_SAM_UNROLL float4 rows on a grid capped at DTC_SAM_MAX_BLOCKS.
#define DTC_SAM_STATE_WORDS 4
#define DTC_SAM_THREADS 256
#define DTC_SAM_UNROLL 4
#define DTC_SAM_MAX_BLOCKS 1024
struct SamKeep {  // layout of the ABI's dtc_sam_keep
  void* live;
  void* saved;
  int64_t bytes;
};
size_t sam_workspace_bytes(int64_t n);
int sam_perturb(float* p, const float* g, float* p_saved, u16* p_bf16, int64_t n, double rho, double eps, int adaptive,
                const float* gmul, const SamKeep* keep, int nkeep, void* state, void* workspace, hipStream_t st);
int sam_restore(float* p, const float* p_saved, u16* p_bf16, int64_t n, const SamKeep* keep, int nkeep,
                const void* state, int* found_inf, hipStream_t st);
int cast_f32_bf16(const float* src, u16* dst, int64_t n, hipStream_t st);
// zero an 8-byte aligned range (a kernel node, unlike hipMemsetAsync's fill dispatch)
int zero_bytes(void* p, size_t bytes, hipStream_t st);
// dst[0:bytes] = src[0:bytes] (16-B aligned) and zp[0:zbytes] = 0 (8-B aligned), one launch
int copy_and_zero(const void* src, void* dst, size_t bytes, void* zp, size_t zbytes, hipStream_t st);
// x[i] *= f (loopback test communicator)
int scale_f32(float* x, int64_t n, float f, hipStream_t st);
// bf16 words in place: x = bf16_rne(widen(x) * f), one fp32 multiply and one rounding (the loopback's bf16 collective)
int scale_bf16(u16* x, int64_t n, float f, hipStream_t st);
int scale_f64(double* x, int64_t n, double f, hipStream_t st);
int scale_i64(int64_t* x, int64_t n, int64_t f, hipStream_t st);
// thread-group communicator: every rank's buffer <- the rank-ordered sum of all (fp32 dtype 0 / int64 2 /
// fp64 3; bf16 dtype 1: the words widened, added in fp32 in rank order and rounded once)
#define DTC_GROUP_MAX 8
struct GroupPtrs { void* p[DTC_GROUP_MAX]; };
int group_sum(const GroupPtrs& g, int w, int64_t n, int dtype, hipStream_t st);
// dst[i] += src[i] (DataParallel reduce-add of replicas sharing a device)
int add_f32(float* dst, const float* src, int64_t n, hipStream_t st);
int amp_check_finite(const float* g, int64_t n, int* found_inf, hipStream_t st);
int amp_scale(const float* x, const float* scale, float* out, int64_t n, hipStream_t st);  // out = x * (*scale)
int amp_update_scale(float* scale, float* inv_scale, int* growth_tracker, int* found_inf, float growth,
                     float backoff, int interval, hipStream_t st);

// ------------------------------------------------------------------ input pipeline
// gather + RandomCrop(pad) + RandomHorizontalFlip + ToTensor + Normalize: uint8 [N][h][w][3] ->
// fp32 [n][3][h][w]; crop = [n][2] offsets (NULL: centre), flip = [n] (NULL: none).
int cifar_augment(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                  const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                  const float* stdv, float* out, int64_t* labels, int* status, hipStream_t st);
// the same launch mixing every row with a partner row of the batch (partner NULL: b - 1 cyclically): mode 1
// Mixup out = A_b * lam + A_p * (1 - lam), mode 2 CutMix out = A_p inside box (y0, y1, x0, x1), A_b outside
int cifar_augment_mix(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                      const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                      const float* stdv, const int32_t* partner, int mode, const float* lam, const uint8_t* box,
                      float* out, int64_t* labels, int64_t* labels_b, int* status, hipStream_t st);
// the plain launch with a chain of n_ops policy ops per image (ops [n][n_ops], args [n][n_ops][6]; RandAugment /
// TrivialAugmentWide, augment_policy.hip) between the flip and Normalize, and an optional erase box [n][4] zeroed
// after it (RandomErasing); writes out (fp32 NCHW) or out_u8 (uint8 NHWC, before Normalize), exactly one of them
int cifar_augment_policy(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                         const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                         const float* stdv, const uint8_t* ops, const float* args, int n_ops, const uint8_t* erase,
                         float* out, uint8_t* out_u8, int64_t* labels, int* status, hipStream_t st);

}  // namespace dtc
