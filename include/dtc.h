/*
 * dtc.h — C ABI of libdtc_amd.so: the MI355X-native (gfx950) kernels and executor for the
 * ResNet-18 / CIFAR-100 data-parallel training step of youngerous/distributed-training-comparison.
 *
 * The reference has no FFI of its own: its operator boundary is the PyTorch module API that
 * src/{single,dp,ddp}/net.py and trainer.py call (nn.Conv2d, nn.BatchNorm2d, F.relu,
 * F.avg_pool2d, nn.Linear, nn.CrossEntropyLoss, optim.SGD, GradScaler, DDP). Every entry
 * point below names the reference call it replaces (file:line under the reference tree).
 *
 * Conventions
 *   - plain C types only; bf16 tensors are uint16_t words (IEEE bfloat16 bit patterns);
 *   - activations are NHWC; conv filters are KRSC ([out][kh][kw][in], in innermost);
 *   - every compute call takes `stream` = a hipStream_t (void* here) and only enqueues work;
 *   - the CALLER owns every device buffer, workspaces included; the library never allocates
 *     or frees caller memory inside a call. Handles (dtc_comm, dtc_net) are library-owned and
 *     released by their destroy function;
 *   - return value: 0 = ok, > 0 = hipError_t / ncclResult_t passed through, < 0 = invalid
 *     argument. dtc_last_error() gives the message (thread-local). Nothing throws or exits;
 *   - reentrant: no unguarded global mutable state; calls for different devices may be made
 *     from different threads (the device is the one current on the calling thread).
 */
#ifndef DTC_AMD_H
#define DTC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTC_ABI_VERSION 1

/* ------------------------------------------------------------------ library */
int dtc_abi_version(void);
const char* dtc_last_error(void);
/* Diagnostics: on SIGSEGV/SIGBUS/SIGFPE/SIGABRT print the faulting native thread (tid, name) and its
 * frames to stderr, then chain to the previous handler (e.g. Python's faulthandler). Idempotent. */
int dtc_install_crash_handler(void);
/* Process-wide kernel tuning knobs (atomic; for benchmarking and A/B measurement). The full list, with
 * defaults and one line each, is the DTC_OPTIONS table in csrc/kernels.h; unknown names return DTC_EINVAL.
 * Examples: "graphs" (0 eager, 1 forward + backward hipGraphs, 2 forward only, 3 backward only,
 * default 4 = auto: the executor captures on first use and replays; any option change invalidates
 * captured graphs), "splitk_ink" (split-K slabs summed in-kernel by the last workgroup of each tile,
 * default 1), "dgrad_s2h" (stride-2 data gradient as a halo sub-pixel conv, default 1), "stem_direct"
 * (plan time: direct 3x3 stem conv, default 1; 0 = im2col + GEMM). */
int dtc_set_option(const char* name, int value);
int dtc_get_option(const char* name);

/* ------------------------------------------------------------------ convolution
 * Replaces nn.Conv2d(bias=False) forward / backward (reference src/ddp/net.py:18-24,
 * net.py:29-35, net.py:91) as launched by autocast (cuDNN in the reference).
 * Requirements: c % 64 == 0, k % 64 == 0, stride in {1, 2} (the 3-channel stem has its own direct
 * kernels, dtc_stem_*; dtc_stem_im2col + a 1x1 "conv" over 64 im2col channels is kept as the
 * stem_direct=0 variant). */
typedef struct {
  int n, h, w, c; /* input  [n][h][w][c]  bf16 */
  int k, r, s;    /* filter [k][r][s][c]  bf16 */
  int stride, pad;
} dtc_conv_desc;

enum { DTC_CONV_FWD = 0, DTC_CONV_DGRAD = 1, DTC_CONV_WGRAD = 2 };

/* bytes of workspace the given pass wants: split-K partial slabs (fp32), and for FWD / DGRAD split-K also
 * the arrival counters of the in-kernel reduction (the last workgroup of each output tile sums the slab;
 * option splitk_ink). 0 is valid for FWD/DGRAD; a workspace with room for the slab only reduces the slab in
 * a separate launch. */
size_t dtc_conv2d_workspace_size(const dtc_conv_desc* d, int pass);
/* y[n][p][q][k] = conv(x, w); if stats != NULL, per-channel (sum, sum^2) of the bf16 output are
 * ADDED into stats — the batch statistics BatchNorm2d needs (net.py:21). A statistics accumulator is
 * dtc_bn_stat_words(k) int64 words, zeroed before its first producer: exact fixed-point sums, so the
 * totals do not depend on the order of the producers' atomic adds (the step is bit-reproducible, as the
 * reference's cudnn.deterministic asks, src/ddp/utils.py:12-13); dtc_bn_stat_totals reads them. */
int dtc_conv2d_fwd(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t* stats,
                   void* ws, size_t ws_bytes, void* stream);
/* Which kernel a conv entry point would launch for this descriptor, request and workspace, and what it would do
 * with the workspace -- read-only: nothing is launched, `ws` is never dereferenced (its address only decides where
 * the 256-byte-aligned arrival counters would sit) and may be NULL. The entry point is named by pass, flags and
 * nprob: FWD -> dtc_conv2d_fwd, with DTC_CONV_ROUTE_SC dtc_conv2d_fwd_sc; DGRAD -> dtc_conv2d_dgrad (RES: a
 * residual is passed), with SC dtc_conv2d_dgrad_sc; WGRAD -> dtc_conv2d_wgrad, with SC dtc_conv2d_wgrad_sc, with
 * nprob 2..4 dtc_conv2d_wgrad_batch. The answer comes from the routing and workspace code those entry points run,
 * under the options in force at the call. Returns non-zero for a descriptor the ABI rejects or a combination that
 * names no entry point. */
enum {
  DTC_CONV_K_GEMM = 0,         /* implicit GEMM */
  DTC_CONV_K_GEMM_CLASSES = 1, /* implicit GEMM, stride-2 DGRAD as four parity classes */
  DTC_CONV_K_C64 = 2,          /* persistent 64 -> 64 channel 3x3 kernel */
  DTC_CONV_K_HALO = 3,         /* halo-tiled 3x3 FWD / DGRAD */
  DTC_CONV_K_DGRAD_S2 = 4,     /* stride-2 3x3 DGRAD as a halo sub-pixel conv */
  DTC_CONV_K_WGRAD_HALO = 5,   /* halo-tiled 3x3 stride-1 WGRAD */
  DTC_CONV_K_WGRAD_S2 = 6      /* halo-tiled 3x3 stride-2 WGRAD (+ shortcut) */
};
enum { DTC_CONV_ROUTE_RES = 1, DTC_CONV_ROUTE_SC = 2 };
typedef struct {
  int kernel;           /* DTC_CONV_K_* */
  int gemm_bm, gemm_bn; /* the GEMM kernels' tile (0 elsewhere) */
  int splits;           /* split-K count asked of the kernel that runs (1: none) */
  int halo_cfg;         /* DTC_CONV_K_HALO: tile configuration (-1 elsewhere) */
  int halo_gen;         /* ... 1: its general tile geometry */
  int reduce_in_kernel; /* 1: a split-K DTC_CONV_K_HALO launch sums its slab itself (the arrival counters fit behind
                           the slab and option splitk_ink is on); 0: no split-K, or a separate reduce launch */
  int sc_ok;            /* the pass has a shortcut-fused launch for this descriptor */
  int refused;          /* 1: the entry point returns an error for this workspace / request and launches nothing */
  int reserved;
  size_t slab_wanted;   /* fp32 slab bytes the pass wants (what the size queries are built on) */
  size_t slab_used;     /* fp32 slab bytes the launch writes, from the start of ws (0: none, or refused) */
} dtc_conv_route;
int dtc_conv2d_route_query(const dtc_conv_desc* d, int pass, int flags, int nprob, const void* ws, size_t ws_bytes,
                           dtc_conv_route* out);
/* dx = conv^T(dy, w) (+ res if non-NULL): the input gradient of Conv2d */
/* 3x3 stride-2 conv (desc) and its BasicBlock's 1x1 stride-2 projection shortcut (net.py:18-19, 29-36) of
 * the same input in one launch: y = conv(x, w), ysc = conv1x1_s2(x, wsc [K][C]); optional BN statistics of
 * each. The shortcut reads exactly the 3x3's centre-tap pixels, so x is read once. Returns
 * DTC_EINVAL for geometries without a fused plan (callers then run the two convs separately). */
int dtc_conv2d_fwd_sc(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t* stats,
                      const uint16_t* wsc, uint16_t* ysc, int64_t* stats_sc, void* stream);
int dtc_conv2d_dgrad(const dtc_conv_desc* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx,
                     const uint16_t* res, void* ws, size_t ws_bytes, void* stream);
/* The same dgrad when dx is the gradient of a post-ReLU BatchNorm output y = relu(bn(x1) [+ bn2(x2)])
 * (net.py:41-44, 108): stores dz = bf16(dx) * [ymask > 0] in dx and ADDS the BN-backward sums into
 * acc1 (and acc2 if x2) exactly as dtc_bn_bwd_reduce does on that dz: the dgrad launch(es), then that
 * reduction in place on dx. dx may alias res. */
int dtc_conv2d_dgrad_bn(const dtc_conv_desc* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx,
                        const uint16_t* res, const uint16_t* ymask, const uint16_t* x1, const float* mean1,
                        const float* invstd1, int64_t* acc1, const uint16_t* x2, const float* mean2,
                        const float* invstd2, int64_t* acc2, void* ws, size_t ws_bytes, void* stream);
/* dx of a projection block's input through conv1 (3x3 stride 2, desc) AND the 1x1 stride-2 shortcut
 * (net.py:18-19, 29-36) in one launch: dx = dgrad(dy, w) + dgrad(dsc, wsc [K][C]); the shortcut's term is
 * nonzero only at the (even, even) pixels and runs as extra reduction steps of that parity class. */
int dtc_conv2d_dgrad_sc(const dtc_conv_desc* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx,
                        const uint16_t* dsc, const uint16_t* wsc, void* stream);
/* dw[k][r][s][c] (fp32) = scale * sum over pixels of dy (x) im2col(x): the weight gradient */
int dtc_conv2d_wgrad(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* dy, float* dw, float scale,
                     void* ws, size_t ws_bytes, void* stream);
/* n (1..4) independent weight gradients of one 3x3 / stride-1 / pad-1 geometry (64-multiple
 * channels) in one halo launch + one reduce launch: dw[i] = scale * wgrad(x[i], dy[i]). The chip is
 * filled by n x splits workgroups, so each gradient's fp32 split-K slab is 1/n the size of a single
 * dtc_conv2d_wgrad's. Replaces the weight-gradient halves of n `nn.Conv2d` backward passes
 * (net.py:18-24, 29-35) that autograd would run one by one. Workspace: ..._batch_workspace_size
 * (0 = no halo plan for this geometry: use dtc_conv2d_wgrad per problem). */
/* The weight gradients of a projection block's 3x3 stride-2 conv1 (desc) and its 1x1 stride-2 shortcut
 * (net.py:18-19, 29-36) in one launch (+ two fixed-order reduces): dw [K][3][3][C] from (x, dy), dw_sc [K][C]
 * from (x, dsc); the shortcut is the centre tap of conv1's operand, so x is read once. Workspace size 0:
 * no fused plan for the geometry (callers then run dtc_conv2d_wgrad for each). */
size_t dtc_conv2d_wgrad_sc_workspace_size(const dtc_conv_desc* d);
int dtc_conv2d_wgrad_sc(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* dy, const uint16_t* dsc, float* dw,
                        float* dw_sc, float scale, void* ws, size_t ws_bytes, void* stream);
size_t dtc_conv2d_wgrad_batch_workspace_size(const dtc_conv_desc* d, int n);
int dtc_conv2d_wgrad_batch(const dtc_conv_desc* d, int n, const uint16_t* const* x, const uint16_t* const* dy,
                           float* const* dw, float scale, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ batch norm (training)
 * Replaces nn.BatchNorm2d train-mode forward/backward (net.py:21,25,37,92) with the F.relu and
 * residual add of BasicBlock.forward (net.py:41-44) and ResNet.forward (net.py:108) fused.
 * x is NHWC bf16 with m = n*h*w pixels and c channels (c % 8 == 0). */
/* Size of one statistics accumulator for c channels, in int64 words (a header word holding the
 * non-finite flag, then 8 slots x 2 statistics x (hi, lo) x c). Zero it before its first producer.
 * Range: a producer's fp32 partial loses its bits below 2^-52 (floor) and must be finite and below 2^40 in
 * magnitude; a partial that is NaN, infinite or FINITE AT OR ABOVE 2^40 (one conv output of 2^20 does that to
 * the sum of squares) is not added and sets the flag instead. A flagged BN yields NaN in every channel: totals,
 * mean / invstd, scale / shift, backward coefficients, dgamma / dbeta and every output element (the fused ReLU
 * keeps NaN). Under AMP the GradScaler skips such a step; in fp32 mode, where there is no GradScaler, the step
 * is not skipped and the loss is NaN. The running statistics of a flagged BN become NaN. Totals stay below
 * 2^55; at most 2^15 partials per slot and channel. */
size_t dtc_bn_stat_words(int c);
/* Host-side read of an accumulator copied to host memory: totals[0][c] = first statistic (sum x / sum dz),
 * totals[1][c] = second (sum x^2 / sum dz*xhat), exactly as the BN kernels form them (NaN if flagged).
 * Pure host code, no device call. */
int dtc_bn_stat_totals(const int64_t* host_words, int c, double* totals);
int dtc_bn_fwd_finalize(int64_t* stats, int c, int64_t count, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                        float eps, float* mean, float* invstd, float* scale, float* shift, void* stream);
int dtc_bn_apply_relu(const uint16_t* x, const float* scale, const float* shift, uint16_t* y, int64_t m, int c,
                      void* stream);
int dtc_bn_apply_add_relu(const uint16_t* x, const float* scale, const float* shift, const uint16_t* res,
                          uint16_t* y, int64_t m, int c, void* stream);
int dtc_bn_apply_dual_relu(const uint16_t* x, const float* scale, const float* shift, const uint16_t* x2,
                           const float* scale2, const float* shift2, uint16_t* y, int64_t m, int c, void* stream);
/* dz = dy * [ymask > 0] (ymask may be NULL: no ReLU); acc1 += (sum dz, sum dz*xhat1) and, if x2,
 * acc2 += (sum dz, sum dz*xhat2); acc* are statistics accumulators (dtc_bn_stat_words(c) int64) */
int dtc_bn_bwd_reduce(const uint16_t* dy, const uint16_t* ymask, const uint16_t* x1, const float* mean1,
                      const float* invstd1, int64_t* acc1, const uint16_t* x2, const float* mean2,
                      const float* invstd2, int64_t* acc2, uint16_t* dz, int64_t m, int c, void* stream);
/* dgamma = gscale*sum dz*xhat, dbeta = gscale*sum dz; coef[3][c] for dtc_bn_bwd_apply; acc re-zeroed */
int dtc_bn_bwd_finalize(int64_t* acc, int c, int64_t count, const float* gamma, const float* mean,
                        const float* invstd, float gscale, float* dgamma, float* dbeta, float* coef, void* stream);
int dtc_bn_bwd_apply(const uint16_t* dz, const uint16_t* x1, const float* coef1, uint16_t* dx1, const uint16_t* x2,
                     const float* coef2, uint16_t* dx2, int64_t m, int c, void* stream);
/* The executor's default forward BN (finalize folded into the apply, one launch): every workgroup folds the
 * statistic slots of its 64 channels (stats: sum x, sum x^2 over `count` elements per channel; read, not
 * re-zeroed) into scale / shift and writes y = relu(bn(x)) (mode 1), relu(bf16(bn(x)) + x2) (mode 2) or
 * relu(bf16(bn(x)) + bf16(bn2(x2))) (mode 3: the projection shortcut's BN, the *2 arguments; NULL otherwise).
 * Side outputs, written once per channel: mean / invstd (saved for the backward), the running statistics
 * (optional; momentum, unbiased variance) and *nbt += 1 (optional). mask_bits (optional, m * c / 8 bytes):
 * the ReLU mask of y, bit k of byte o / 8 = [y[o + k] > 0] for element offset o. c % 64 == 0. */
int dtc_bn_fin_apply(int mode, const uint16_t* x, const int64_t* stats, int64_t count, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, int64_t* nbt, float momentum,
                     float eps, float* mean, float* invstd, const uint16_t* x2, const int64_t* stats2,
                     const float* gamma2, const float* beta2, float* running_mean2, float* running_var2,
                     int64_t* nbt2, float* mean2, float* invstd2, uint16_t* y, uint8_t* mask_bits, int64_t m, int c,
                     void* stream);
/* The executor's default BN backward, driven by the forward's mask bits: dz = dy * bit (stored to dz_out if
 * non-NULL; dz_out may alias dy), dgamma = gscale * sum dz*xhat, dbeta = gscale * sum dz (both optional) and
 * dx = gamma*invstd * (dz - sum dz / count - xhat * sum dz*xhat / count), for one BN (x2 == NULL) or for
 * the two BNs that share dz in a projection block (x2 ... dx2). one_launch == 0: a reduction into `acc`
 * ((1 or 2) * dtc_bn_stat_words(c) int64 words, zeroed by the caller; they hold the sums afterwards) and an
 * apply that folds them; one_launch != 0: one launch, one workgroup per 8 channels, acc unused -- only for
 * m <= 4096 (2048 with a second BN), DTC_EINVAL beyond. c % 64 == 0, c <= 2048. */
int dtc_bn_bwd_mask(const uint16_t* dy, const uint8_t* mask_bits, uint16_t* dz_out, const uint16_t* x1,
                    const float* gamma1, const float* mean1, const float* invstd1, float* dgamma1, float* dbeta1,
                    uint16_t* dx1, const uint16_t* x2, const float* gamma2, const float* mean2, const float* invstd2,
                    float* dgamma2, float* dbeta2, uint16_t* dx2, int64_t count, float gscale, int one_launch,
                    int64_t* acc, size_t acc_words, int64_t m, int c, void* stream);

/* ------------------------------------------------------------------ stem, head, loss
 * stem: self.conv1 = nn.Conv2d(3, 64, 3, 1, 1) (net.py:91) as im2col [n*h*w][64] + GEMM.
 * head: F.avg_pool2d(out, 4) + view + self.linear (net.py:113-115), global pool.
 * loss: nn.CrossEntropyLoss() (trainer.py:40, 155), mean reduction. */
int dtc_stem_im2col(const float* x_nchw, uint16_t* cols, int n, int h, int w, void* stream);
int dtc_stem_pack_weight(const uint16_t* w27, uint16_t* w64, int k, void* stream);
/* Direct stem conv (the executor's default): y [n*h*w][64] bf16 = conv1(x) from fp32 NCHW x and the
 * bf16 KRSC weight [64][27], the 27 taps gathered per 256-pixel tile into LDS (no im2col matrix in
 * HBM); stats (optional, dtc_bn_stat_words(64) int64, accumulated) = BN batch sums of the bf16 outputs. The
 * weight gradient dw27 [64][27] fp32 = scale * sum_pixels dy (x) taps(x), workspace from
 * dtc_stem_wgrad_workspace_size. */
int dtc_stem_fwd(const float* x_nchw, const uint16_t* w27, uint16_t* y, int64_t* stats, int n, int h, int w,
                 void* stream);
size_t dtc_stem_wgrad_workspace_size(int n, int h, int w);
int dtc_stem_wgrad(const float* x_nchw, const uint16_t* dy, float* dw27, float scale, int n, int h, int w, void* ws,
                   size_t ws_bytes, void* stream);
int dtc_head_fwd(const uint16_t* act, int n, int hw, int c, const uint16_t* wfc, const float* bfc, int ncls,
                 float* feat, float* logits, void* stream);
size_t dtc_head_bwd_workspace_size(int n, int c, int ncls);
int dtc_head_bwd(const float* dlogits, const float* feat, const uint16_t* wfc, int n, int hw, int c, int ncls,
                 float scale, float* dw, float* db, uint16_t* dact, void* ws, size_t ws_bytes, void* stream);
int dtc_xent_fwd(const float* logits, const int64_t* labels, int n, int ncls, float* loss, float* lse,
                 void* stream);
/* The training step's loss in one launch (n <= 4096): loss and lse as dtc_xent_fwd (bit-identical), plus
 * scaled = loss * (*scale) when scaled != NULL (GradScaler.scale) and the loss stored into host_loss (a
 * pinned, device-accessible host word; NULL = none) -- read after an event recorded behind the launch. */
int dtc_xent_fwd_ex(const float* logits, const int64_t* labels, int n, int ncls, float* loss, float* lse,
                    const float* scale, float* scaled, float* host_loss, void* stream);
int dtc_xent_bwd(const float* logits, const int64_t* labels, const float* lse, const float* gscale, int n, int ncls,
                 float* dlogits, void* stream);
/* Soft targets: label smoothing, Mixup and CutMix as one loss. The target of row b is the distribution
 *   q_b = (1 - smoothing) * (lam[b] * onehot(labels_a[b]) + (1 - lam[b]) * onehot(labels_b[b])) + smoothing / ncls
 * (nn.CrossEntropyLoss(label_smoothing=) on the two-hot target torchvision's MixUp / CutMix produce), so with
 * l_b the row's log-sum-exp
 *   loss      = mean_b (l_b - (1 - smoothing) * (lam z[ya] + (1 - lam) z[yb]) - (smoothing / ncls) * sum_j z[b][j])
 *   dlogits   = (exp(z[b][j] - l_b) - q_b[j]) * (*gscale) / n            (gscale NULL: 1)
 * labels_b == NULL and lam == NULL (both or neither, else DTC_EINVAL): label smoothing only, lam = 1, yb = ya.
 * labels_a[b] == labels_b[b] puts both terms on one class. A label outside [0, ncls) makes the loss NaN, as in
 * dtc_xent_fwd, and hits no class in the gradient; a lam outside [0, 1] (or NaN) makes the loss NaN.
 * smoothing outside [0, 1]: DTC_EINVAL, nothing is launched. dtc_xent_soft_fwd_ex is one launch with
 * dtc_xent_fwd_ex's outputs (n <= 4096); lse is bit-identical to dtc_xent_fwd_ex's, and with smoothing = 0 and
 * no labels_b so are the loss (finite logits) and dtc_xent_soft_bwd's dlogits to dtc_xent_bwd's. */
int dtc_xent_soft_fwd_ex(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                         float smoothing, int n, int ncls, float* loss, float* lse, const float* scale, float* scaled,
                         float* host_loss, void* stream);
/* loss and lse as dtc_xent_soft_fwd_ex without the row cap, two launches (dtc_xent_fwd's form; lse bit-identical,
 * the loss equal to rounding: the row sums are formed in another order) */
int dtc_xent_soft_fwd(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      float smoothing, int n, int ncls, float* loss, float* lse, void* stream);
int dtc_xent_soft_bwd(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      float smoothing, const float* lse, const float* gscale, int n, int ncls, float* dlogits,
                      void* stream);
/* Evaluation metrics of one batch (reference trainer.py validate / test: `criterion(pred, label).item()` and
 * utils.py:18-31 `accuracy(pred, label, topk)`), one launch of one workgroup, no host synchronisation: writes
 * *rec (device memory, 16 bytes) and nothing else. 1 <= n <= 4096, ncls >= 1, 1 <= topk <= ncls.
 *   loss        mean cross-entropy over the n rows, bit-identical to what dtc_xent_fwd stores in *loss (an
 *               out-of-range label makes it NaN, as there);
 *   n           the row count;
 *   top1, topk  rows whose label has rank < 1 / rank < topk, where for a label y in range
 *                 rank = #{ j != y : !(z[j] <= z[y]) } + #{ j < y : z[j] == z[y] }
 *               (strictly greater logits first, ties to the lower index, a NaN logit above everything; a NaN
 *               label logit gives rank ncls - 1). A row whose label is out of range counts for neither.
 *               torch.topk leaves the order of ties unspecified; on tie-free rows the two agree. */
typedef struct dtc_eval_record {
  float loss;
  int32_t n, top1, topk;
} dtc_eval_record; /* 16 bytes */
int dtc_eval_metrics(const float* logits, const int64_t* labels, int n, int ncls, int topk, dtc_eval_record* rec,
                     void* stream);

/* ------------------------------------------------------------------ optimizer / AMP
 * sgd: optim.SGD(lr, weight_decay, momentum, nesterov=True).step() (trainer.py:92-98, 158) over a
 * flat fp32 buffer; grads are multiplied by *inv_scale (GradScaler.unscale_) and the step is skipped
 * when *found_inf != 0 (GradScaler.step); p_bf16 receives the bf16 shadow of the new parameters.
 * p, g and momentum_buf 16-byte aligned, p_bf16 8-byte aligned, n a positive multiple of 4 (else DTC_EINVAL).
 * amp: GradScaler's _amp_foreach_non_finite_check_and_unscale_ / _amp_update_scale_ (main.py:25). */
int dtc_sgd_nesterov_flat(float* p, const float* g, float* momentum_buf, uint16_t* p_bf16, int64_t n, float lr,
                          float weight_decay, float momentum, const float* inv_scale, const int* found_inf,
                          void* stream);
/* adam: torch.optim.Adam (decoupled = 0: g += weight_decay * p) / torch.optim.AdamW (decoupled = 1:
 * p *= 1 - lr * weight_decay) with amsgrad = False, maximize = False -- the optimizer the reference's README
 * suggests trying in configure_optimizers (trainer.py:91-107) -- over flat fp32 buffers p, g, exp_avg m,
 * exp_avg_sq v (all 16-byte aligned, n % 4 == 0); p_bf16 (8-byte aligned) receives the bf16 shadow. As for sgd,
 * grads are multiplied by *inv_scale (NULL: 1) and the whole step is skipped when *found_inf != 0 (NULL: never).
 * `state` is dtc_adam_state_words() (= 4) 32-bit words of device memory, 16-byte aligned, zeroed by the caller
 * before the first step and owned by the library's kernels afterwards: word 0 is the int32 count of steps
 * taken. It advances on the device, and only on a step that is not skipped (torch's GradScaler does not
 * advance state['step'] on a skipped step either), so the bias corrections 1 - beta^t need no host
 * synchronisation. Two launches: a one-thread tick that advances the count and derives lr / (1 - beta1^t) and
 * sqrt(1 - beta2^t) in double, then the update. The scalars are doubles because torch's are Python floats:
 * 1 - beta2 formed from a float 0.999 is off by 4.7e-5. Requires eps > 0, betas in [0, 1), lr, weight_decay >= 0. */
int dtc_adam_state_words(void);
int dtc_adam_flat(float* p, const float* g, float* exp_avg, float* exp_avg_sq, uint16_t* p_bf16, int64_t n, void* state,
                  double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                  const float* inv_scale, const int* found_inf, void* stream);
/* torch.nn.utils.clip_grad_norm_(norm_type = 2) over a flat gradient buffer (16-byte aligned, n % 4 == 0) that
 * may still be loss-scaled: *total_norm = s * sqrt(sum g^2) and *grad_mult = s * min(1, max_norm / (*total_norm
 * + 1e-6)) with s = *inv_scale (NULL: 1), both fp32 words in device memory. Passing grad_mult as the inv_scale
 * of dtc_sgd_nesterov_flat / dtc_adam_flat applies unscale and clip inside the update: the gradients are not
 * rewritten. Squares are summed in double in a fixed order (no floating-point atomics): bit-identical results run
 * to run. Non-finite gradients give a non-finite norm (error_if_nonfinite = False); found_inf is not touched.
 * workspace: dtc_grad_norm_workspace_bytes(n) bytes, 8-byte aligned, overwritten. Two launches (the read pass
 * and a one-workgroup finalize), no host synchronisation. Requires max_norm > 0. */
size_t dtc_grad_norm_workspace_bytes(int64_t n);
int dtc_grad_norm_clip(const float* g, int64_t n, const float* inv_scale, double max_norm, void* workspace,
                       float* total_norm, float* grad_mult, void* stream);
/* Segment plan: where each parameter tensor lies in the flat buffers (p, g, optimizer state and the bf16 shadow
 * share one layout), for the per-tensor reductions and LARS below. Segments are given in strictly increasing,
 * non-overlapping order; offset is a non-negative multiple of 4 elements, numel >= 1 (any value: linear.bias with
 * 10 classes has 10 elements), flags bit 0 = ADAPT (the trust ratio and weight decay apply; clear for BatchNorm
 * weights / biases and linear.bias), every other flag bit and `reserved` zero, 1 <= nseg <= 4096. Anything else:
 * DTC_EINVAL and *out = NULL. dtc_segplan_create is pure host code (no device call): the handle holds the table and
 * the work map derived from it, one entry per chunk of dtc_segplan_chunk_elems() elements of one segment.
 * dtc_segplan_device_bytes: the device memory the plan wants (the two tables, one partial slot of two doubles per
 * chunk, the per-segment results), a multiple of 16. dtc_segplan_bind uploads the tables into such a region (16-byte
 * aligned, caller-owned, to be kept until the plan is destroyed or bound elsewhere), enqueued on `stream`: once per
 * model, the only copy -- nothing is copied per step. A plan serves one stream at a time (its slots are reused). */
typedef struct { int64_t offset, numel; int32_t flags; int32_t reserved; } dtc_seg; /* flags bit 0: ADAPT */
#define DTC_SEG_ADAPT 1
typedef struct dtc_segplan dtc_segplan;
int dtc_segplan_create(dtc_segplan** out, const dtc_seg* segs_host, int nseg);
int dtc_segplan_destroy(dtc_segplan* plan);
int dtc_segplan_num_segments(const dtc_segplan* plan);
int64_t dtc_segplan_chunk_elems(void);
size_t dtc_segplan_device_bytes(const dtc_segplan* plan);
int dtc_segplan_bind(dtc_segplan* plan, void* dev, size_t bytes, void* stream);
/* Per-tensor L2 norms of p and g (16-byte aligned flat buffers covering every segment): seg_out (optional, device
 * fp32 [nseg][3]) = (||p_s||, |mult| * ||g_s||, ratio_s) with mult = *gmul (NULL: 1). Squares are summed in double
 * in a fixed order -- per thread in index order, a butterfly over the wave, the waves in index order, one slot per
 * chunk, the slots in index order -- so the result is bit-identical from run to run; each norm is rounded to fp32
 * once. Elements outside the segments are not read. Here ratio_s is the bare ||p_s|| / (|mult| ||g_s||) of an ADAPT
 * segment, and 1 where a norm is zero and for the other segments. Two launches, no host synchronisation. */
int dtc_seg_norms(dtc_segplan* plan, const float* p, const float* g, const float* gmul, float* seg_out, void* stream);
/* lars: LARS (You et al. 2017) = SGD with momentum whose step is scaled per tensor by a trust ratio; with
 * momentum 0.9 and nesterov it is the reference's optimizer (trainer.py:92-98) plus that ratio. With mult =
 * *inv_scale (NULL: 1; GradScaler's 1/scale or dtc_grad_norm_clip's grad_mult), for every segment s:
 *   wn = ||p_s||, gn = |mult| * ||g_s||                                       (as dtc_seg_norms)
 *   ADAPT:      ratio = trust_coef * wn / (gn + weight_decay * wn + eps), with trust_clip != 0 (LARC's "clip" mode)
 *               min(ratio / lr, 1); ratio = 1 when wn or gn is zero; rounded once to fp32;
 *               d = (g * mult + weight_decay * p) * ratio
 *   otherwise:  ratio = 1 and no weight decay;  d = g * mult
 *   buf = momentum * buf + d ;  u = nesterov ? d + momentum * buf : buf ;  p -= lr * u ;  p_bf16 = bf16(p)
 * The whole step is skipped when *found_inf != 0 (NULL: never): p, momentum_buf and p_bf16 stay bit-unchanged.
 * Elements outside the segments are neither read nor written. The norms are recomputed from the buffers at every
 * call. seg_out (optional) as for dtc_seg_norms, ratio_s being the ratio applied. Three launches (norm pass, ratios,
 * update), no host synchronisation, no floating-point atomics, bit-identical from run to run. Requires lr,
 * weight_decay, eps >= 0, momentum in [0, 1), trust_coef > 0, lr > 0 with trust_clip; p, g, momentum_buf 16-byte
 * aligned, p_bf16 8-byte aligned; a bound plan. */
int dtc_lars_flat(dtc_segplan* plan, float* p, const float* g, float* momentum_buf, uint16_t* p_bf16, double lr,
                  double weight_decay, double momentum, int nesterov, double trust_coef, double eps, int trust_clip,
                  const float* inv_scale, const int* found_inf, float* seg_out, void* stream);
/* ema: an exponential moving average of the weights (timm ModelEma, torchvision's --model-ema,
 * tf.train.ExponentialMovingAverage) over 1..4 flat ranges in ONE update launch -- a model's parameters and its
 * BatchNorm running statistics together. Per element of every range
 *   ema += (src - ema) * w   (one fused multiply-add);   ema_bf16 = bf16(ema) where ema_bf16 != NULL
 *                             (dtc_cast_f32_bf16's rounding: the EMA's own GEMM-operand shadow)
 * with w = (float)(1 - decay), or with warmup != 0 w = (float)(1 - min(decay, (1 + t) / (10 + t))), formed in double
 * and rounded once, t being the count of updates including this one. `state` is dtc_ema_state_words() (= 4) 32-bit
 * words of device memory, 16-byte aligned, zeroed by the caller before the first call: word 0 is the int32 count t
 * of updates applied, word 1 the fp32 w of the last update, the rest reserved. When *found_inf != 0 (NULL: never)
 * nothing happens: ema, ema_bf16 and state stay bit-unchanged -- a skipped optimizer step is not an update. Two
 * launches (a one-thread tick that advances t and writes w, then the update, its blocks shared among the ranges in
 * proportion to their lengths), no host synchronisation, no atomics, bit-identical from run to run; 14 bytes of
 * HBM traffic per element with a bf16 copy. Requires (else DTC_EINVAL, before any device call): 1 <= nranges <= 4;
 * n a positive multiple of 4; ema and src 16-byte, ema_bf16 8-byte aligned; [ema, ema + n) overlapping neither
 * [src, src + n) nor another entry's ema; decay in [0, 1). */
typedef struct { float* ema; const float* src; uint16_t* ema_bf16; int64_t n; } dtc_ema_range;
int dtc_ema_state_words(void);
int dtc_ema_update(const dtc_ema_range* ranges, int nranges, void* state, double decay, int warmup,
                   const int* found_inf, void* stream);
/* grad_accum: gradient accumulation over one fp32 range (torch's `.grad +=` over the micro-batches of one optimizer
 * step, DistributedDataParallel.no_sync()). The backward kernels write their gradients, so the running sum of a
 * window lives in a second buffer `acc`; per element
 *   DTC_ACCUM_STORE (1)   acc = g         (the first micro-batch of a window)         8 bytes of HBM traffic
 *   DTC_ACCUM_ADD (2)     acc = acc + g   (every further one inside the window)      12
 *   DTC_ACCUM_FINISH (3)  g = g + acc     (the micro-batch that closes the window)   12
 * Each result is exactly one IEEE fp32 add (round to nearest even, no FMA, nothing reassociated): the window's sum is
 * bit-defined, g_N + ((g_1 + g_2) + ... + g_N-1) for the micro-batches 1..N in order, and an inf or NaN of any
 * micro-batch reaches the final g, so dtc_amp_check_finite over g after FINISH still decides a skipped step. The operand that is not the destination stays bit-unchanged. One launch, 16-byte vector
 * loads and stores, no atomics, no host synchronisation; every element is written by exactly one thread, so the
 * result is bit-identical from run to run. Requires (else DTC_EINVAL, before any device call): n a positive multiple
 * of 4; acc and g non-NULL and 16-byte aligned; mode in 1..3; [acc, acc + n) and [g, g + n) not overlapping. */
enum { DTC_ACCUM_OFF = 0, DTC_ACCUM_STORE = 1, DTC_ACCUM_ADD = 2, DTC_ACCUM_FINISH = 3 };
int dtc_grad_accum_flat(float* acc, float* g, int64_t n, int mode, void* stream);
/* bf16 gradient compression for the bucketed all-reduce (torch's default_hooks.bf16_compress_hook), one launch each:
 *   compress    c[i] = bf16_rne(acc ? g[i] + acc[i] : g[i])   4 (+ 4) bytes read, 2 written per element
 *   decompress  g[i] = widen(c[i])  (bits << 16: exact; NaN payloads, inf, -0 and subnormals preserved)   2 read, 4 written
 * The rounding is dtc_cast_f32_bf16's, round to nearest even: a NaN stays a NaN, a finite value at or above the bf16
 * overflow threshold becomes +-inf. With acc != NULL the sum is exactly one IEEE fp32 add (no FMA, nothing
 * reassociated) followed by the one rounding, so the result is bit-identical to dtc_grad_accum_flat(DTC_ACCUM_FINISH)
 * followed by the plain compress, at 10 instead of 18 bytes per element. compress never writes g or acc, decompress
 * never writes c. 16-byte fp32 loads and stores; compress stores 16 bytes of bf16 from c's first 16-byte boundary on,
 * with an 8-byte store for the 4 elements in front of it and for a last 4 left over; decompress loads 8 bytes of bf16
 * per 16-byte store; no atomics; every element is written by exactly one thread. Requires (else DTC_EINVAL, before any device call): n a positive multiple of 4; g, c non-NULL;
 * g and acc 16-byte aligned, c 8-byte aligned; [c, c + n) overlapping neither [g, g + n) nor [acc, acc + n). */
int dtc_grad_compress_bf16(const float* g, const float* acc, uint16_t* c, int64_t n, void* stream);
int dtc_grad_decompress_bf16(const uint16_t* c, float* g, int64_t n, void* stream);
/* psgd: PowerSGD rank-r gradient compression (Vogels et al. 2019; torch's ddp_comm_hooks.powerSGD_hook) on the flat
 * gradient buffer, run after a local backward. The plan is built from a table of tensors in strictly increasing,
 * non-overlapping order: offset a non-negative multiple of 4 elements, rows, cols >= 1 with rows * cols not
 * overflowing, 0 <= rank <= min(rows, cols, 4) (rank 0: the tensor is all-reduced as it is), reserved zero,
 * 1 <= n <= 4096; anything else: DTC_EINVAL and *out = NULL. dtc_psgd_plan_create is pure host code.
 * dtc_psgd_plan_numel(what): DTC_PSGD_P the elements of all P blocks (sum rows * rank), DTC_PSGD_Q of all Q blocks
 * (sum cols * rank), DTC_PSGD_UNCOMPRESSED of the rank-0 tensors, DTC_PSGD_STAGING = uncompressed + P,
 * DTC_PSGD_QSTRIDE the Q count rounded up to a multiple of 4. dtc_psgd_plan_device_bytes / dtc_psgd_plan_bind as
 * for dtc_segplan (tables, the back-project slots of doubles, arrival counters and per-tensor marks; 16-byte aligned
 * region; the only copy). Caller-owned fp32 buffers, 16-byte aligned: g (gradients) and e (error feedback, flat
 * layout, zeroed before the first step; NULL: none), staging [DTC_PSGD_STAGING] = [uncompressed | P], q
 * [2][DTC_PSGD_QSTRIDE] -- q[0] the warm start (filled by the caller before the first step: the same values on every
 * rank), q[1] the working copy -- and `state`, 4 int32 words zeroed before the first step (word 0: the next warm
 * start is q[1], not q[0]; word 1: the last step was non-finite; the host need not read either). One step, every
 * compressed tensor seen as a row-major rows x cols matrix, A = g + e (one fp32 add), one launch per call:
 *   dtc_psgd_orthonormalize(DTC_PSGD_Q)  Qh = orthonormalize(state[0] ? q[1] : q[0]) -> q[1]; the source -> q[0]
 *   dtc_psgd_project                     P = A Qh; staging = [the rank-0 tensors | P]
 *        -- the caller all-reduces (SUM) staging, DTC_PSGD_STAGING elements --
 *   dtc_psgd_orthonormalize(DTC_PSGD_P)  Ph = orthonormalize(P) in staging; notes a non-finite P
 *   dtc_psgd_backproject                 Q = A^T Ph -> q[1]
 *        -- the caller all-reduces (SUM) q[1] = q + DTC_PSGD_QSTRIDE, DTC_PSGD_Q elements --
 *   dtc_psgd_reconstruct                 gh = Ph Q^T -> g;  e = __fsub_rn(__fadd_rn(g, e), __fmul_rn(c, gh)) (c: 1 /
 *                                        world size; bit-defined, no contraction); rank-0 tensors staging -> g
 * orthonormalize is modified Gram-Schmidt dividing by (norm + epsilon); norm + epsilon == 0 gives a zero column
 * (torch gives NaN), and a column whose norm fell to 2^-20 of its norm before the projections -- it lay in the span
 * of its predecessors, what is left is rounding noise -- is divided by that earlier norm, so it stays negligible. Dot products are summed in double in a fixed order and rounded to fp32 once; the back-project
 * splits the rows over workgroups with one slot per chunk, folded in index order. No floating-point atomics: every
 * result is bit-identical from run to run. Elements between the tensors are neither read nor written.
 * If the all-reduced P or Q holds a non-finite value (the same verdict on every rank) dtc_psgd_reconstruct writes NaN
 * into the compressed tensors' gradients and leaves e bit-unchanged, q[0] holds the warm start as before the step and
 * state[0] = 0 selects it for the next; after a finite step state[0] = 1. No host synchronisation. Requires (else
 * DTC_EINVAL, before any device call): non-NULL, 16-byte aligned pointers (e may be NULL); a bound plan; what in
 * {DTC_PSGD_Q, DTC_PSGD_P}; epsilon >= 0; 0 < c <= 1. A plan serves one stream at a time. */
typedef struct { int64_t offset, rows, cols; int32_t rank; int32_t reserved; } dtc_psgd_tensor;
enum { DTC_PSGD_P = 0, DTC_PSGD_Q = 1, DTC_PSGD_UNCOMPRESSED = 2, DTC_PSGD_STAGING = 3, DTC_PSGD_QSTRIDE = 4 };
typedef struct dtc_psgd_plan dtc_psgd_plan;
int dtc_psgd_plan_create(dtc_psgd_plan** out, const dtc_psgd_tensor* tensors_host, int n);
int dtc_psgd_plan_destroy(dtc_psgd_plan* plan);
int64_t dtc_psgd_plan_numel(const dtc_psgd_plan* plan, int what);
size_t dtc_psgd_plan_device_bytes(const dtc_psgd_plan* plan);
int dtc_psgd_plan_bind(dtc_psgd_plan* plan, void* dev, size_t bytes, void* stream);
int dtc_psgd_orthonormalize(dtc_psgd_plan* plan, int what, float* q, float* staging, int* state, double epsilon,
                            void* stream);
int dtc_psgd_project(dtc_psgd_plan* plan, const float* g, const float* e, const float* q, float* staging,
                     void* stream);
int dtc_psgd_backproject(dtc_psgd_plan* plan, const float* g, const float* e, const float* staging, float* q,
                         void* stream);
int dtc_psgd_reconstruct(dtc_psgd_plan* plan, float* g, float* e, const float* staging, const float* q, int* state,
                         double c, void* stream);
/* sam: sharpness-aware minimisation (SAM, Foret et al. 2021) and its scale-adaptive form (ASAM, Kwon et al. 2021)
 * over the whole flat buffers (n a positive multiple of 4; alignment padding holds zeros in p and g and so is not
 * moved). dtc_sam_perturb, after the first backward, with m = *gmul (NULL: 1; GradScaler's 1 / scale):
 *   t_i  = g_i (adaptive == 0)  |  p_i * g_i (adaptive != 0)
 *   S    = sum t_i^2 in double, in dtc_grad_norm_clip's fixed order;  gn = |m| * sqrt(S)
 *   ok   = isfinite(S) && isfinite(m);  coef = ok ? (float)(rho * m / (gn + eps)) : 0   (double, rounded once)
 *   state = {float coef; float norm = (float)gn; int32 skipped = !ok; int32 reserved}
 *   every element:  p_saved_i = p_i
 *   ok:   p_i = p_i + coef * g_i  |  p_i + (coef * g_i) * (p_i * p_i), each operation one IEEE fp32 rounding (no
 *         FMA); an element whose increment is zero keeps its bits;  p_bf16_i = bf16(p_i) (dtc_cast_f32_bf16's rounding)
 *   !ok:  p and p_bf16 stay bit-unchanged (g is not multiplied in: 0 * NaN is NaN)
 *   keep[k]: saved <- live, raw 8-byte words (BatchNorm running statistics and batch counts across the second forward)
 * dtc_sam_restore, after the second backward and ahead of the optimizer step: p_i = p_saved_i and p_bf16_i =
 * bf16(p_i) for every element -- a copy, never a subtraction, so the weights return bit for bit; keep[k]: live <-
 * saved; and *found_inf = 1 if found_inf != NULL and state.skipped (the word is never cleared here): GradScaler then
 * skips the step and backs the scale off, with no host synchronisation.
 * `state`: dtc_sam_state_words() (= 4) 32-bit words of device memory, 16-byte aligned, written by every perturb.
 * `workspace`: dtc_sam_workspace_bytes(n) bytes, 8-byte aligned, overwritten. Launches: perturb three (the norm pass,
 * which does not read p unless adaptive and carries the keep copies; a one-workgroup finalize; the update), restore
 * one. HBM traffic per element: norm 4 bytes (adaptive 8), update 18, restore 10. 16-byte loads and stores, no
 * floating-point atomics, every element written by exactly one thread: bit-identical from run to run. Requires (else
 * DTC_EINVAL, before any device call): non-NULL p, g, p_saved, p_bf16, state, workspace; n a positive multiple of 4;
 * p, g, p_saved 16-byte and p_bf16 8-byte aligned; [p_saved, p_saved + n) overlapping neither p nor g; rho >= 0,
 * eps > 0; 0 <= nkeep <= DTC_SAM_MAX_KEEP, every keep record with non-NULL 8-byte aligned live and saved, bytes a
 * positive multiple of 8, and no range of the table overlapping another. */
#define DTC_SAM_MAX_KEEP 4
typedef struct { void* live; void* saved; int64_t bytes; } dtc_sam_keep;
int dtc_sam_state_words(void);
size_t dtc_sam_workspace_bytes(int64_t n);
int dtc_sam_perturb(float* p, const float* g, float* p_saved, uint16_t* p_bf16, int64_t n, double rho, double eps,
                    int adaptive, const float* gmul, const dtc_sam_keep* keep, int nkeep, void* state, void* workspace,
                    void* stream);
int dtc_sam_restore(float* p, const float* p_saved, uint16_t* p_bf16, int64_t n, const dtc_sam_keep* keep, int nkeep,
                    const void* state, int* found_inf, void* stream);
int dtc_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);
int dtc_amp_check_finite(const float* g, int64_t n, int* found_inf, void* stream);
/* GradScaler.scale(loss): out = x * (*scale) with the scale device-resident (no host sync) */
int dtc_amp_scale(const float* x, const float* scale, float* out, int64_t n, void* stream);
int dtc_amp_update_scale(float* scale, float* inv_scale, int* growth_tracker, int* found_inf, float growth_factor,
                         float backoff_factor, int growth_interval, void* stream);

/* ------------------------------------------------------------------ input pipeline
 * Replaces the host DataLoader workers' per-sample transforms (src/ddp/dataset.py:43-64:
 * RandomCrop(32, padding=4) -> RandomHorizontalFlip -> ToTensor -> Normalize) and the
 * Subset/DistributedSampler gather (dataset.py:95-98) with one launch per batch.
 * images: uint8 [n_images][h][w][3] in device memory; targets: int64 [n_images] (may be NULL when
 * labels is NULL); index: int64 [n] dataset rows (NULL: 0..n-1); crop: uint8 [n][2] (row, col)
 * offsets into the zero-padded image, each in [0, 2*pad] (NULL: pad, pad = no crop shift);
 * flip: uint8 [n], non-zero = mirror (NULL: none); mean/std: HOST pointers to 3 floats;
 * out: fp32 [n][3][h][w]; labels: int64 [n] (NULL: skip); status: device int set to 1 when an index
 * is out of range or an offset exceeds 2*pad (that image is written as zeros before normalize,
 * label 0); never cleared by the call (NULL: skip). Requires w % 4 == 0 and h*w*3 <= 12 KiB. */
int dtc_cifar_augment(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                      const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                      const float* std, float* out, int64_t* labels, int* status, void* stream);

/* dtc_cifar_augment plus Mixup / CutMix in the same launch (torchvision.transforms.v2.MixUp / CutMix: the
 * augmented batch mixed with a permutation of itself). With A_b what dtc_cifar_augment writes for row b
 * (index, crop, flip of b) and p = partner[b] (int32 [n], a row of THIS batch; NULL: (b + n - 1) % n, i.e.
 * batch.roll(1, 0)), the partner keeping its own crop and flip:
 *   mode 1 (Mixup):  out[b] = A_b * lam[b] + A_p * (1 - lam[b])   lam fp32 [n]; two rounded fp32 products and one
 *                    rounded add, 1 - lam[b] formed in fp32
 *   mode 2 (CutMix): out[b] = A_p inside box[b], A_b outside      box uint8 [n][4] = (y0, y1, x0, x1), half open,
 *                    in output coordinates
 * labels[b] = targets[index[b]], labels_b[b] = targets[index[p]] (int64 [n] outputs, NULL: skip). Both uint8
 * source images of a row are staged in LDS and the batch is written once. status is also set, and the row
 * written unmixed (labels_b[b] = labels[b]), when partner[b] is outside [0, n), the box is inverted or leaves
 * the image, or lam is outside [0, 1]. Other arguments, conditions and shape limits as dtc_cifar_augment. */
int dtc_cifar_augment_mix(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                          const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                          const float* std, const int32_t* partner, int mode, const float* lam, const uint8_t* box,
                          float* out, int64_t* labels, int64_t* labels_b, int* status, void* stream);

/* dtc_cifar_augment with an augmentation policy (RandAugment / TrivialAugmentWide) and RandomErasing in the same
 * launch: gather, crop, flip, then n_ops (0..4) ops per image on the uint8 image, then ToTensor / Normalize, then
 * the erase box set to 0.0f. ops: uint8 [n][n_ops] op codes; args: fp32 [n][n_ops][6], the op's g0..g5 (both may be
 * NULL when n_ops == 0); erase: uint8 [n][4] = (y0, y1, x0, x1), half open, output coordinates (NULL: none; an empty
 * box is legal). Exactly one of out (fp32 [n][3][h][w]) and out_u8 (uint8 [n][h][w][3], the image before
 * Normalize -- what a following dtc_cifar_augment_mix takes as its `images`, with index = crop = flip = NULL and
 * targets = this call's labels) is non-NULL; erase needs out. All randomness is the caller's. With a the current
 * image, every fp32 expression evaluated as written (no fused multiply-add), conversions to uint8 clamping to
 * [0, 255] and then truncating:
 *   0 Identity
 *   1 Affine (nearest, fill 0): X = ox + 0.5f - 0.5f*w, Y = oy + 0.5f - 0.5f*h; sx = (g0*X + g1*Y) + g2,
 *     sy = (g3*X + g4*Y) + g5; rx = rintf(sx + (0.5f*w - 0.5f)), ry = rintf(sy + (0.5f*h - 0.5f)); a[ry][rx] when
 *     0 <= rx <= w-1 and 0 <= ry <= h-1, else 0
 *   2 Brightness g0*a + g1*0      3 Color g0*a + g1*gray, gray = trunc((0.2989f*R + 0.587f*G) + 0.114f*B)
 *   4 Contrast g0*a + g1*m, m = (float)(sum of gray over the image) / (float)(h*w)
 *   5 Sharpness g0*a + g1*blur; blur = a on the border, (8 neighbours + 5*centre + 6) / 13 in integers inside
 *   6 Posterize a & (int)g0       7 Solarize (float)a >= g0 ? 255 - a : a
 *   8 AutoContrast, per channel with lo / hi its min / max: a when lo == hi, else
 *     trunc(clamp(((float)a - lo) * (255.0f / (float)(hi - lo))))
 *   9 Equalize, per channel: step = (h*w - hist[last non-empty bin]) / 255; a when step == 0, else
 *     min(255, (exclusive_cumsum(hist)[a] + step/2) / step)
 * status is also set when an op code is above 9, an arg that the op reads is not finite or Posterize's g0 is no
 * integer in [0, 255] (that op then acts as Identity), or an erase box is inverted or leaves the image (not
 * applied). Other arguments, conditions and shape limits as dtc_cifar_augment. */
int dtc_cifar_augment_policy(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                             const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                             const float* std, const uint8_t* ops, const float* args, int n_ops, const uint8_t* erase,
                             float* out, uint8_t* out_u8, int64_t* labels, int* status, void* stream);

/* ------------------------------------------------------------------ RCCL communicator
 * Replaces the NCCL traffic of DistributedDataParallel (trainer.py:31): the construction-time
 * parameter broadcast, the per-forward buffer broadcast and the bucketed gradient all-reduce.
 * Bootstrap: rank 0 calls dtc_comm_get_unique_id, the id travels over the existing
 * torch.distributed rendezvous (init_process_group, ddp/main.py:18-23), every rank calls
 * dtc_comm_init. dtype: 0 = fp32, 1 = bf16, 2 = int64, 3 = fp64. */
typedef struct dtc_comm dtc_comm;
size_t dtc_comm_unique_id_bytes(void);
int dtc_comm_get_unique_id(void* out);
int dtc_comm_init(dtc_comm** out, int rank, int world, const void* unique_id, int device);
int dtc_comm_allreduce_sum(dtc_comm* comm, void* buf, size_t count, int dtype, void* stream);
int dtc_comm_broadcast(dtc_comm* comm, void* buf, size_t count, int dtype, int root, void* stream);
int dtc_comm_destroy(dtc_comm* comm);
/* torch.distributed.barrier() (reference ddp/trainer.py:156, dp/single variants have none): returns
 * once every rank called it and this rank's work enqueued on `stream` before the call has finished
 * (torch's NCCL barrier = a one-element all-reduce + a stream synchronize). One float is SUM
 * all-reduced on the communicator's side stream; the host polls the completion event (no sleeping
 * driver wait: the GPU is idle until the host returns). comm == NULL or a loopback communicator:
 * the stream drain alone. */
int dtc_barrier(dtc_comm* comm, void* stream);
/* Test communicator (no RCCL): every all-reduce through it -- dtc_comm_allreduce_sum, the Reducer's
 * bucket all-reduces inside dtc_rn18_backward and SyncBN's statistics all-reduces -- multiplies the
 * buffer by `factor` on the stream the collective would run on (the side stream for buckets) and
 * appends (address, count, is_async) to a host log; broadcast is the identity; the communicator
 * reports `world` ranks. With factor == world it is `world` ranks holding identical data. Lets a
 * one-GPU test prove that every gradient bucket is reduced exactly once and only after its producers,
 * and that SyncBN's sums really go through the collective (a one-rank RCCL SUM is the identity and
 * proves neither). fp32 / bf16 / int64 / fp64 buffers (int64 x the integer factor; a bf16 word becomes
 * bf16_rne(widen(word) * factor): one fp32 multiply, one round-to-nearest-even). */
int dtc_comm_init_loopback(dtc_comm** out, int device, int world, float factor);
int dtc_comm_log_size(dtc_comm* comm);
int dtc_comm_log_entry(dtc_comm* comm, int idx, uint64_t* addr, uint64_t* count, int* is_async);
int dtc_comm_log_clear(dtc_comm* comm);
/* In-process thread-group communicator (test transport, no RCCL): `world` handles outs[0..world-1] =
 * ranks 0..world-1 on one device, each driven by its own host thread with its own streams and buffers.
 * Collectives are matched by call order (as RCCL's): the calling thread blocks until every rank issued
 * the same collective (kind, count, dtype, root; a mismatch or a 120 s wait is an error for all ranks),
 * then the data really moves between the ranks' buffers on a group stream that waits for every rank's
 * producers -- SUM all-reduce as the rank-ordered fp32/int64/fp64 sum written into every buffer (bf16 buffers: the
 * words widened, added in fp32 in rank order without FMA and rounded once to nearest even), broadcast as
 * root -> all copies, barrier as a host rendezvous + stream drain -- and each rank's consumer stream
 * (the Reducer's side stream for buckets) waits for the result. Lets one GPU run W ranks with DISTINCT
 * data through the product Reducer, broadcasts and SyncBN (max 8 ranks). Every all-reduce is logged
 * as for the loopback communicator. Destroy each handle with dtc_comm_destroy. */
int dtc_comm_init_thread_group(dtc_comm** outs, int world, int device);
int dtc_comm_rank(const dtc_comm* comm);
int dtc_comm_world(const dtc_comm* comm);

/* ------------------------------------------------------------------ DataParallel group
 * Replaces the per-step traffic of nn.DataParallel (reference src/dp/trainer.py:27):
 * replicate = broadcast of the module's flat buffers from device_ids[0] to every replica (C5),
 * backward = reduce-add of the replicas' flat gradient buffers onto device_ids[0] (C7), input scatter
 * / logits gather as peer copies (C6). One process drives all devices: distinct devices get one RCCL
 * rank each (ncclCommInitAll) and every call is one grouped RCCL collective over all replicas;
 * replicas that all share ONE device (device_ids=[0, 0], the single-GPU test form) run the same
 * calls as on-device copies and a fixed-order HIP reduce-add kernel. bufs[i] / streams[i] belong to
 * replica i (its device), bufs[0] is the root. dtype as for dtc_comm_*. */
typedef struct dtc_dp dtc_dp;
int dtc_dp_create(dtc_dp** out, int n, const int* devices);
int dtc_dp_destroy(dtc_dp* group);
int dtc_dp_is_local(const dtc_dp* group);
int dtc_dp_broadcast(dtc_dp* group, void* const* bufs, size_t count, int dtype, void* const* streams);
int dtc_dp_reduce_add(dtc_dp* group, float* const* bufs, size_t count, void* const* streams);
/* dst (on dst_device) <- src (on src_device), `bytes`, ordered on `stream` (hipMemcpyPeerAsync; a plain
 * device-to-device copy when the devices are equal) */
int dtc_copy_peer(void* dst, int dst_device, const void* src, int src_device, size_t bytes, void* stream);

/* ------------------------------------------------------------------ ResNet-18 executor
 * The whole forward (ResNet.forward, net.py:107-116) and backward of ResNet18() (net.py:119-120)
 * as one call each, for a fixed per-rank batch and input size. Parameters live in ONE flat fp32
 * buffer laid out in reverse registration order (so backward produces gradients in increasing
 * address order and DDP buckets are contiguous); conv weights are stored KRSC and exposed to
 * Python as strided [k][c][r][s] views. dtc_rn18_param_info lists the 62 parameters in
 * registration order (net.py:86-105) with names identical to ResNet18().state_dict() keys. */
typedef struct dtc_net dtc_net;
int dtc_rn18_create(dtc_net** out, int batch, int height, int width, int num_classes, float bucket_cap_mb);
int dtc_rn18_destroy(dtc_net* net);
int dtc_rn18_num_params(const dtc_net* net);
int dtc_rn18_param_info(const dtc_net* net, int idx, const char** name, int64_t* offset, int64_t* numel, int* ndim,
                        int64_t* shape4, int64_t* stride4);
int64_t dtc_rn18_flat_numel(const dtc_net* net);
/* BN buffers: running_mean/running_var in one fp32 flat buffer; num_batches_tracked in an int64 array */
int dtc_rn18_num_bn(const dtc_net* net);
int dtc_rn18_bn_info(const dtc_net* net, int idx, const char** prefix, int* channels, int64_t* mean_offset,
                     int64_t* var_offset);
int64_t dtc_rn18_bufs_numel(const dtc_net* net);
size_t dtc_rn18_workspace_bytes(const dtc_net* net);
int dtc_rn18_num_buckets(const dtc_net* net);
int dtc_rn18_bucket_info(const dtc_net* net, int idx, int64_t* offset, int64_t* numel);
/* Precision of the executor (call before dtc_rn18_bind; re-plans the workspace): 0 = bf16 activations
 * with fp32 accumulation and master weights (the reference under --amp, autocast, trainer.py:152-159),
 * 1 = fp32 throughout (the reference without --amp, ddp/trainer.py:160-165): fp32 activations in the
 * workspace, f32-input MFMA convolutions, BN / pool / Linear on fp32 tensors with the fp32 master
 * weights (no bf16 shadow), no autocast rounding points. */
int dtc_rn18_set_precision(dtc_net* net, int fp32);
int dtc_rn18_precision(const dtc_net* net);
/* Attach caller-owned device memory. Zeroes the workspace statistics areas (enqueued on stream). */
int dtc_rn18_bind(dtc_net* net, void* workspace, float* params, float* grads, uint16_t* params_bf16, float* bufs,
                  int64_t* num_batches_tracked, void* stream);
/* x: NCHW fp32 [batch][3][h][w]; logits fp32 [batch][ncls]. train != 0: batch statistics +
 * running-stat update; train == 0: running statistics (eval mode).
 * Graph mode (option "graphs"): everything after the input im2col is captured once per train flag
 * (on an internal stream) and replayed into `stream`; logits are copied out of the workspace. The
 * backward is captured as segments split at bucket boundaries, with the all-reduces issued eagerly
 * between segment replays; re-captured when grad_scale or the presence of comm changes, and after
 * dtc_rn18_bind. Capture mode (dtc_rn18_enable_capture) runs eagerly. */
int dtc_rn18_forward(dtc_net* net, const float* x, float* logits, int train, void* stream);
/* Gradients of every parameter, scaled by grad_scale (1/world for DDP's mean), written (not
 * accumulated) into the bound flat grad buffer. If comm != NULL each bucket is all-reduced (sum)
 * on the communicator's side stream as soon as backward has produced it; the call returns with
 * `stream` ordered after the last all-reduce. Must follow a training-mode dtc_rn18_forward (one
 * backward per forward: the forward saves the activations and zeroes the BN backward sums). */
int dtc_rn18_backward(dtc_net* net, const float* dlogits, float grad_scale, dtc_comm* comm, void* stream);
/* SyncBatchNorm (replaces nn.SyncBatchNorm.convert_sync_batchnorm(model), torch/nn/modules/
 * batchnorm.py, the conversion README.md:40 recommends; not called by the reference trainers).
 * comm != NULL: every training-mode BN all-reduces its per-channel partial sums (exact int64) over `comm`
 * (forward: sum x, sum x^2; backward: sum dz, sum dz*xhat) on the compute stream and normalises
 * with the global element count (running_var's unbiased factor too); dgamma/dbeta keep this
 * rank's share (x 1/world) so the Reducer's mean matches DDP over SyncBatchNorm. Use a
 * communicator of its own, not the one passed to dtc_rn18_backward. Disables graph replay.
 * comm == NULL: per-rank statistics (the reference's BatchNorm2d). */
int dtc_rn18_set_sync_bn(dtc_net* net, dtc_comm* comm);
/* Gradient accumulation inside the backward (dtc_grad_accum_flat's modes; host only, no device call). Sticky: `mode`
 * applies to every later dtc_rn18_backward, dtc_rn18_xent_backward and dtc_rn18_xent_soft_backward, in both
 * precisions, until the next call; dtc_rn18_bind resets it to DTC_ACCUM_OFF. `acc`: caller-owned device memory of
 * dtc_rn18_flat_numel floats in the gradient buffer's layout, 16-byte aligned, not overlapping the bound gradients
 * (DTC_EINVAL otherwise); NULL only with DTC_ACCUM_OFF. The work is done per gradient bucket, at the point of the
 * backward where the bucket's gradients are complete, on the stream that holds both of its producers (the
 * weight-gradient stream when weight gradients are pending, else the compute stream), so it overlaps the rest of
 * the backward:
 *   STORE / ADD  acc = g / acc = acc + g over the bucket's range. The backward must be given comm == NULL
 *                (DTC_EINVAL before any launch otherwise): nothing is all-reduced -- DDP's no_sync().
 *   FINISH       g = g + acc over the bucket's range immediately before the bucket's all-reduce (comm != NULL), which
 *                therefore reduces the accumulated gradient; without a communicator the add alone.
 *   OFF          the backward as without this call: same launches, streams and results.
 * A backward whose mode is not OFF always runs eagerly (as with SyncBN); it neither captures nor drops graphs, so
 * alternating modes from step to step causes no re-capture. The accumulate launches take no profiling slot. */
int dtc_rn18_set_grad_accum(dtc_net* net, float* acc, int mode);
/* bf16 gradient compression of the bucket all-reduces (host only, no device call). Sticky like
 * dtc_rn18_set_grad_accum; dtc_rn18_bind resets it to DTC_COMPRESS_OFF. `staging`: caller-owned device memory of
 * dtc_rn18_flat_numel bf16 words in the gradient buffer's element layout, 16-byte aligned, not overlapping the bound
 * gradients; NULL only with DTC_COMPRESS_OFF. Gradients must be bound first; an unknown mode is DTC_EINVAL.
 * DTC_COMPRESS_BF16 and a backward with comm != NULL: at each bucket point, on the stream that holds both producers,
 * one dtc_grad_compress_bf16 launch over the contiguous range of the buckets complete there into staging (with
 * DTC_ACCUM_FINISH the fused form with acc, in place of the FINISH launch), then each bucket's all-reduce on its
 * staging range as bf16 -- half the bytes of the fp32 one; its placement (options comm_on_side, comm_tail_inline) is
 * decided as without compression -- and one dtc_grad_decompress_bf16 per bucket into the gradients, enqueued directly
 * behind that bucket's collective on the stream the collective runs on, so the end-of-backward join orders the compute
 * stream after it: the finiteness check, clipping, LARS and the optimizers read ordinary fp32 gradients (a value that
 * overflowed to inf in bf16 arrives as inf). With comm == NULL (no communicator; STORE / ADD micro-steps) nothing is
 * compressed, staging is not touched and the gradients are bit-identical to DTC_COMPRESS_OFF. A backward whose mode
 * is not OFF always runs eagerly; it neither captures nor drops graphs. dtc_rn18_comm_timing's events keep bracketing
 * the collective alone; the new launches take no profiling slot. SyncBN's statistics are not compressed. */
enum { DTC_COMPRESS_OFF = 0, DTC_COMPRESS_BF16 = 1 };
int dtc_rn18_set_grad_compress(dtc_net* net, uint16_t* staging, int mode);
/* CrossEntropyLoss backward fused with the network backward (the reference's
 * `scaler.scale(loss).backward()`, ddp/trainer.py:157, when the loss is nn.CrossEntropyLoss of the
 * network's logits, trainer.py:40,155): dlogits = (softmax(logits) - onehot(labels)) * (*gscale) / N
 * written into the executor's own dlogits buffer, then dtc_rn18_backward on it -- one call, so the
 * two launches reach the GPU back to back (this runs right after the per-step barrier, when the GPU
 * queue is empty). logits [batch][num_classes] fp32, labels int64 [batch], lse = the per-row
 * log-sum-exp dtc_xent_fwd wrote, gscale: device fp32 scalar or NULL (1). */
int dtc_rn18_xent_backward(dtc_net* net, const float* logits, const int64_t* labels, const float* lse,
                           const float* gscale, float grad_scale, dtc_comm* comm, void* stream);
/* The same call for soft targets (dtc_xent_soft_bwd's dlogits; lse from dtc_xent_soft_fwd_ex), under the same
 * rule: computed inside the head backward kernel when the backward runs eagerly and option xent_fuse != 0,
 * otherwise one dtc_xent_soft_bwd launch into the executor's dlogits buffer, then dtc_rn18_backward. With
 * smoothing = 0 and labels_b = lam = NULL every gradient is bit-identical to dtc_rn18_xent_backward's. */
int dtc_rn18_xent_soft_backward(dtc_net* net, const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                                const float* lam, float smoothing, const float* lse, const float* gscale,
                                float grad_scale, dtc_comm* comm, void* stream);
/* One evaluation batch (reference trainer.py validate / test: `net(img)` in eval mode, the loss and
 * `accuracy`) as one call with no host synchronisation: the eval-mode forward (running statistics) of the
 * first n_valid images of x, then dtc_eval_metrics over their logits and labels into *rec (device memory).
 * 1 <= n_valid <= batch (and <= 4096); exactly n_valid images of x and n_valid labels are read. The remaining
 * batch - n_valid image slots of the executor's own input are zeroed; eval-mode rows are independent, so the
 * valid rows' logits do not depend on that padding -- a short last batch runs on the full-batch executor.
 * logits: fp32 [batch][num_classes] (rows >= n_valid are the padding's), or NULL = a workspace region.
 * The BatchNorm coefficients of all layers are computed by one launch; the other launches are those of
 * dtc_rn18_forward(train = 0). Always runs eagerly (option "graphs" does not apply), takes no profiling slots,
 * both precisions. Leaves parameters, running statistics and num_batches_tracked untouched; overwrites the
 * saved mean / invstd of every BatchNorm, so a backward of an earlier training forward must not follow. */
int dtc_rn18_eval_batch(dtc_net* net, const float* x, const int64_t* labels, int n_valid, int topk, float* logits,
                        dtc_eval_record* rec, void* stream);
/* dtc_rn18_eval_batch reading the parameters, their bf16 shadow and the running statistics from the three given
 * buffers (e.g. an EMA of the weights, dtc_ema_update) instead of the bound ones: the bound buffers' layout, all
 * three non-NULL, params and params_bf16 16-byte aligned as for dtc_rn18_bind. The bound buffers are neither read
 * nor written and stay bound; no graph is dropped or captured (always eager, both precisions -- the fp32 executor
 * does not read params_bf16). Everything else, the overwritten saved mean / invstd included, as dtc_rn18_eval_batch. */
int dtc_rn18_eval_batch_weights(dtc_net* net, const float* params, const uint16_t* params_bf16, const float* bufs,
                                const float* x, const int64_t* labels, int n_valid, int topk, float* logits,
                                dtc_eval_record* rec, void* stream);
/* Byte offset into the workspace of the executor's own fp32 [batch][num_classes] dlogits buffer.
 * A caller that writes the loss gradient there (e.g. the fused cross-entropy backward) and passes
 * that pointer to dtc_rn18_backward saves the graph path's copy-in. */
int dtc_rn18_dlogits_buffer(const dtc_net* net, size_t* ws_offset);

/* Per-layer activations held in the workspace after dtc_rn18_forward (NHWC bf16 except the
 * fp32 "head.feat_f32"): name, byte offset into the workspace, {n, h, w, c}. For parity tests. */
int dtc_rn18_num_activations(const dtc_net* net);
int dtc_rn18_activation_info(const dtc_net* net, int idx, const char** name, size_t* ws_offset, int* shape4);
/* Opt-in (before dtc_rn18_bind): keep copies of the backward's activation gradients per block
 * ("grad.layer2.0.dz", ".dc2", ".ds", ".da1", ".dz1", ".dc1", ".dxs", ".dx", "grad.stem.dz/dc") in
 * extra workspace, for teacher-forced per-layer parity tests. */
int dtc_rn18_enable_capture(dtc_net* net);
int dtc_rn18_num_captures(const dtc_net* net);
int dtc_rn18_capture_info(const dtc_net* net, int idx, const char** name, size_t* ws_offset, int* shape4);
/* Live timing of every convolution call of training steps (forward, dgrad, wgrad incl. split-K
 * reductions) between begin and end. Each call's kernels stamp the first workgroup start and the
 * last workgroup end (s_memrealtime, converted with hipDeviceAttributeWallClockRate) into a device
 * slot; the backward folds the slots into device totals once per step (graph-safe, no host work
 * per call). begin() arms it (first call: allocation + graph re-capture; later calls: totals
 * re-zeroed; `capacity` > 0 is unused), end() synchronizes the device, returns per-pass totals
 * (index 0 = forward, 1 = dgrad, 2 = wgrad: ms, algorithmic FLOPs, calls) and disarms. */
int dtc_rn18_profile_begin(dtc_net* net, int capacity);
int dtc_rn18_profile_end(dtc_net* net, double* ms_by_kind, double* flops_by_kind, int* count_by_kind);
/* The same with nkinds (1..4) entries per array; kind 3 = the BatchNorm family of the mask-bit path
 * (forward finalize+apply, backward reduce, backward finalize+apply), work = algorithmic HBM bytes
 * (every tensor the kernel must touch, read or written once: the in-step BN HBM roofline). */
int dtc_rn18_profile_end_ex(dtc_net* net, int nkinds, double* ms_by_kind, double* work_by_kind, int* count_by_kind);
/* Event timing of the same launcher calls (bench.py's roofline): while profiling is armed and `pairs` > 0,
 * every timed launcher call of an EAGER step whose weight gradients run on the compute stream (options
 * graphs = 0, bwd_streams = 0) is bracketed by two timing events on the compute stream (at most `pairs`
 * calls; `pairs` = 0 switches it off). _result synchronises, sums the elapsed times (ms) and algorithmic
 * work per kind as profile_end_ex does, and resets. */
int dtc_rn18_profile_events(dtc_net* net, int pairs);
int dtc_rn18_profile_events_result(dtc_net* net, int nkinds, double* ms_by_kind, double* work_by_kind,
                                   int* count_by_kind);
/* Timed launcher calls since the last dtc_rn18_profile_events() that were NOT bracketed because the event
 * pool was used up (`pairs` too small for the region): their durations are missing from _result's totals,
 * so a caller reporting a roofline from them must refuse it when this is non-zero. */
int dtc_rn18_profile_events_dropped(dtc_net* net, long long* dropped);
/* Communication timing of the DDP backward (the first multi-GPU run must be diagnosable by
 * itself): the next `steps` backward calls that carry a communicator record timing events -- the backward's
 * start and the Reducer's join on the compute stream, each bucket collective's start / end on the stream it
 * runs on, the compute stream's wait for the weight-gradient stream (collectives of the earlier buckets and
 * the remaining weight gradients) before the stem weight gradient, and the tail from the last backward kernel
 * to the join (the last bucket's collective). steps = 0 disarms. _result synchronises and returns means over
 * the recorded steps: bucket_us[3 * i + 0 / 1 / 2] = start / end offset from the backward's start and the
 * collective's duration for bucket i < max_buckets (issue order); exposed_us[0] = tail (last kernel -> join),
 * [1] = the weight-gradient join wait, [2] = [0] + [1], [3] = the backward's duration, [4] = steps with a
 * join recorded (eager backward); *steps = steps recorded. Then disarms and frees the events. */
int dtc_rn18_comm_timing(dtc_net* net, int steps);
int dtc_rn18_comm_timing_result(dtc_net* net, int max_buckets, double* bucket_us, double* exposed_us, int* steps);

#ifdef __cplusplus
}
#endif
#endif /* DTC_AMD_H */
