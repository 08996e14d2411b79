// Sharpness-aware minimisation (SAM, Foret et al. 2021; ASAM, Kwon et al. 2021) on the flat buffers: the step that
// moves the weights to the (approximately) worst point of the rho-ball around them, and the step that brings them
// back. Between the two the caller runs a second forward / backward; the base optimizer then steps at the restored
// weights with the gradient taken at the perturbed ones.
//     perturb   t = g (plain) | p * g (adaptive);  S = sum t^2 (double, fixed order);  gn = |m| * sqrt(S)
//               coef = fp32(rho * m / (gn + eps)), m = *gmul (GradScaler's 1/scale; NULL: 1)
//               p_saved = p;  p += coef * g  |  p += (coef * g) * (p * p);  p_bf16 = bf16(p)
//     restore   p = p_saved;  p_bf16 = bf16(p)          (a copy, never a subtraction: the weights return bit for bit)
// A non-finite S or m makes the perturbation a no-op (coef = 0 is not multiplied in: 0 * NaN is NaN) and sets
// `skipped` in the device record, which the restore turns into *found_inf = 1: GradScaler then skips the step and
// backs the scale off, with no host synchronisation. Up to DTC_SAM_MAX_KEEP small ranges (BatchNorm running
// statistics and batch counts, ~38 KB) are saved by the perturb and put back by the restore as raw 8-byte words, so
// the second forward's update of them is undone; they ride in the norm launch and the restore launch.
// Launches: perturb = norm pass (4 B per element read, 8 B adaptive) + one-workgroup finalize + update (4 p + 4 g
// read, 4 p_saved + 4 p + 2 bf16 written = 18 B); restore = one (4 read, 4 + 2 written = 10 B). HBM-bound.
// The sum is grad_sumsq_kernel's (optim.hip): per thread in index order, block_sum_ordered, one slot per workgroup,
// the slots in index order by one thread. No floating-point atomics, vector stores only, every element written by
// exactly one thread: bit-identical from run to run. Each perturbed element is fl(p + fl(coef * g)), adaptive
// fl(p + fl(fl(coef * g) * fl(p * p))): explicit IEEE operations, nothing contracted.
#include "../../include/dtc.h"
#include "flat.h"
#include "kernels.h"

namespace dtc {

struct SamState {
  float coef;   // rho * m / (gn + eps) of the last perturb (0 when skipped)
  float norm;   // gn of the last perturb
  int skipped;  // 1: S or m was not finite, the weights were not moved
  int reserved;
};
static_assert(sizeof(SamState) == 4 * DTC_SAM_STATE_WORDS, "SamState is DTC_SAM_STATE_WORDS 32-bit words");

constexpr int SAM_NORM_THREADS = 1024;  // grad_sumsq_kernel's shape: one workgroup fills a CU, few slots
constexpr int SAM_NORM_MAX_BLOCKS = 256;
constexpr int SAM_THREADS = DTC_SAM_THREADS, SAM_UNROLL = DTC_SAM_UNROLL, SAM_MAX_BLOCKS = DTC_SAM_MAX_BLOCKS;

static int sam_norm_blocks(int64_t n) { return flat_blocks(n / 4, SAM_NORM_THREADS, SAM_NORM_MAX_BLOCKS); }
size_t sam_workspace_bytes(int64_t n) { return n > 0 ? (size_t)sam_norm_blocks(n) * sizeof(double) : 0; }

// the keep ranges of one launch, by value: dst <- src, `words` 8-byte words each
struct SamKeepTable {
  uint2* dst[DTC_SAM_MAX_KEEP];
  const uint2* src[DTC_SAM_MAX_KEEP];
  int64_t words[DTC_SAM_MAX_KEEP];
  int n;
};
template <int THREADS>
__device__ __forceinline__ void sam_keep_copy(const SamKeepTable& keep) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int k = 0; k < keep.n; ++k)
    for (int64_t i = blockIdx.x * (int64_t)THREADS + threadIdx.x; i < keep.words[k]; i += stride)
      keep.dst[k][i] = keep.src[k][i];
}

template <bool ADAPTIVE>
__device__ __forceinline__ double sam_sumsq4(double acc, const f32x4& g, const f32x4& p) {
  if (!ADAPTIVE) return sumsq4(acc, g);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double t = (double)p[k] * (double)g[k];  // exact: 24 + 24 bits
    acc += t * t;
  }
  return acc;
}

// the plain form never reads p
template <bool ADAPTIVE>
__global__ void __launch_bounds__(SAM_NORM_THREADS) sam_sumsq_kernel(const float* __restrict__ g,
                                                                     const float* __restrict__ p, int64_t n4,
                                                                     double* __restrict__ slots,
                                                                     const SamKeepTable keep) {
  const int64_t stride = (int64_t)gridDim.x * SAM_NORM_THREADS;
  const f32x4* __restrict__ g4 = (const f32x4*)g;
  const f32x4* __restrict__ p4 = (const f32x4*)p;
  double acc[1] = {0.0};
  int64_t i = blockIdx.x * (int64_t)SAM_NORM_THREADS + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {  // four (adaptive: eight) loads in flight per thread per trip
    const f32x4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
    f32x4 pa = a, pb = b, pc = c, pd = d;
    if (ADAPTIVE) pa = p4[i], pb = p4[i + stride], pc = p4[i + 2 * stride], pd = p4[i + 3 * stride];
    acc[0] = sam_sumsq4<ADAPTIVE>(acc[0], a, pa);
    acc[0] = sam_sumsq4<ADAPTIVE>(acc[0], b, pb);
    acc[0] = sam_sumsq4<ADAPTIVE>(acc[0], c, pc);
    acc[0] = sam_sumsq4<ADAPTIVE>(acc[0], d, pd);
  }
  for (; i < n4; i += stride) {
    const f32x4 a = g4[i];
    f32x4 pa = a;
    if (ADAPTIVE) pa = p4[i];
    acc[0] = sam_sumsq4<ADAPTIVE>(acc[0], a, pa);
  }
  sam_keep_copy<SAM_NORM_THREADS>(keep);
  block_sum_ordered<SAM_NORM_THREADS>(acc);
  if (threadIdx.x == 0) slots[blockIdx.x] = acc[0];
}

__global__ void __launch_bounds__(64) sam_finalize_kernel(const double* __restrict__ slots, int nslots,
                                                          const float* __restrict__ gmul, double rho, double eps,
                                                          SamState* __restrict__ state) {
  __shared__ double sh[SAM_NORM_MAX_BLOCKS];
#pragma unroll
  for (int k = threadIdx.x; k < SAM_NORM_MAX_BLOCKS; k += 64) sh[k] = k < nslots ? slots[k] : 0.0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;  // index order; the unused slots add + 0.0, which changes no bit of a sum of squares
#pragma unroll 16
  for (int k = 0; k < SAM_NORM_MAX_BLOCKS; ++k) s += sh[k];
  const double m = gmul ? (double)*gmul : 1.0;
  const double gn = fabs(m) * sqrt(s);
  const bool ok = isfinite(s) && isfinite(m);
  SamState out;
  out.coef = ok ? (float)(rho * m / (gn + eps)) : 0.f;
  out.norm = (float)gn;
  out.skipped = ok ? 0 : 1;
  out.reserved = 0;
  *state = out;
}

// e == 0 leaves p's bits alone (-0 + +0 is +0): rho = 0 and a zero gradient move nothing
__device__ __forceinline__ float sam_add(float p, float e) { return e != 0.f ? __fadd_rn(p, e) : p; }

template <bool ADAPTIVE>
__global__ void __launch_bounds__(SAM_THREADS) sam_update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ saved, u16* __restrict__ pb,
                                                                 int64_t n4, const SamState* __restrict__ state) {
  const float coef = state->coef;
  const bool move = state->skipped == 0;  // uniform over the grid
  f32x4* __restrict__ p4 = (f32x4*)p;
  const f32x4* __restrict__ g4 = (const f32x4*)g;
  f32x4* __restrict__ s4 = (f32x4*)saved;
  f32x4 pv[SAM_UNROLL], gv[SAM_UNROLL];
  stream_chunks<SAM_THREADS, SAM_UNROLL>(
      n4,
      [&](int k, int64_t base, uint32_t i) {
        pv[k] = (p4 + base)[i];
        gv[k] = (g4 + base)[i];
      },
      [&](int k, int64_t base, uint32_t i) {
        (s4 + base)[i] = pv[k];
        if (move) {
          f32x4 q = pv[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float d = __fmul_rn(coef, gv[k][e]);
            if (ADAPTIVE) d = __fmul_rn(d, __fmul_rn(q[e], q[e]));
            q[e] = sam_add(q[e], d);
          }
          (p4 + base)[i] = q;
          store_bf16x4(pb + base * 4 + i * 4u, q);
        }
      });
}

__global__ void __launch_bounds__(SAM_THREADS) sam_restore_kernel(float* __restrict__ p,
                                                                  const float* __restrict__ saved,
                                                                  u16* __restrict__ pb, int64_t n4,
                                                                  const SamState* __restrict__ state,
                                                                  int* __restrict__ found_inf,
                                                                  const SamKeepTable keep) {
  if (found_inf && blockIdx.x == 0 && threadIdx.x == 0 && state->skipped) *found_inf = 1;  // never cleared here
  f32x4* __restrict__ p4 = (f32x4*)p;
  const f32x4* __restrict__ s4 = (const f32x4*)saved;
  f32x4 sv[SAM_UNROLL];
  stream_chunks<SAM_THREADS, SAM_UNROLL>(
      n4, [&](int k, int64_t base, uint32_t i) { sv[k] = (s4 + base)[i]; },
      [&](int k, int64_t base, uint32_t i) {
        (p4 + base)[i] = sv[k];
        store_bf16x4(pb + base * 4 + i * 4u, sv[k]);
      });
  sam_keep_copy<SAM_THREADS>(keep);
}

// keep[k] checked and laid into the table: to_saved = the perturb's direction (saved <- live)
static int sam_keep_table(const char* fn, const SamKeep* keep, int nkeep, bool to_saved, SamKeepTable* tab) {
  DTC_CHECK_ARG(nkeep >= 0 && nkeep <= DTC_SAM_MAX_KEEP, "%s: nkeep = %d outside [0, %d]", fn, nkeep,
                DTC_SAM_MAX_KEEP);
  DTC_CHECK_ARG(nkeep == 0 || keep, "%s: null pointer (keep)", fn);
  *tab = SamKeepTable{};
  tab->n = nkeep;
  for (int k = 0; k < nkeep; ++k) {
    const SamKeep& q = keep[k];
    DTC_CHECK_ARG(q.live && q.saved, "%s: keep %d: null pointer (live or saved)", fn, k);
    DTC_CHECK_ARG(aligned(q.live, 8) && aligned(q.saved, 8), "%s: keep %d: live and saved must be 8-byte aligned", fn,
                  k);
    DTC_CHECK_ARG(q.bytes > 0 && q.bytes % 8 == 0, "%s: keep %d: bytes = %lld must be a positive multiple of 8", fn,
                  k, (long long)q.bytes);
    DTC_CHECK_ARG(!ranges_overlap(q.live, q.bytes, q.saved, q.bytes), "%s: keep %d: live and saved overlap", fn, k);
    for (int o = 0; o < k; ++o)
      DTC_CHECK_ARG(!ranges_overlap(q.saved, q.bytes, keep[o].saved, keep[o].bytes) &&
                        !ranges_overlap(q.saved, q.bytes, keep[o].live, keep[o].bytes) &&
                        !ranges_overlap(q.live, q.bytes, keep[o].saved, keep[o].bytes) &&
                        !ranges_overlap(q.live, q.bytes, keep[o].live, keep[o].bytes),
                    "%s: keep %d and keep %d overlap", fn, o, k);
    tab->dst[k] = (uint2*)(to_saved ? q.saved : q.live);
    tab->src[k] = (const uint2*)(to_saved ? q.live : q.saved);
    tab->words[k] = q.bytes / 8;
  }
  return 0;
}

#define SAM_NONNULL(fn, x) DTC_CHECK_ARG(x, "%s: null pointer (%s)", fn, #x)

static int sam_flat_args(const char* fn, const float* p, const float* saved, const u16* pb, int64_t n) {
  DTC_CHECK_ARG(mult4(n), "%s: n = %lld must be a positive multiple of 4", fn, (long long)n);
  DTC_CHECK_ARG(aligned(p, 16) && aligned(saved, 16), "%s: p and p_saved must be 16-byte aligned", fn);
  DTC_CHECK_ARG(aligned(pb, 8), "%s: p_bf16 must be 8-byte aligned", fn);
  DTC_CHECK_ARG(!ranges_overlap(saved, n * 4, p, n * 4), "%s: p_saved overlaps p", fn);
  return 0;
}

int sam_perturb(float* p, const float* g, float* p_saved, u16* p_bf16, int64_t n, double rho, double eps, int adaptive,
                const float* gmul, const SamKeep* keep, int nkeep, void* state, void* workspace, hipStream_t st) {
  SAM_NONNULL("sam_perturb", p);
  SAM_NONNULL("sam_perturb", g);
  SAM_NONNULL("sam_perturb", p_saved);
  SAM_NONNULL("sam_perturb", p_bf16);
  SAM_NONNULL("sam_perturb", state);
  SAM_NONNULL("sam_perturb", workspace);
  DTC_TRY(sam_flat_args("sam_perturb", p, p_saved, p_bf16, n));
  DTC_CHECK_ARG(aligned(g, 16), "sam_perturb: g must be 16-byte aligned");
  DTC_CHECK_ARG(!ranges_overlap(p_saved, n * 4, g, n * 4), "sam_perturb: p_saved overlaps g");
  DTC_CHECK_ARG(aligned(state, 16) && aligned(workspace, 8),
                "sam_perturb: state must be 16-byte aligned, the workspace 8-byte aligned");
  DTC_CHECK_ARG(rho >= 0.0, "sam_perturb: rho = %g must not be negative", rho);  // (false for a NaN too)
  DTC_CHECK_ARG(eps > 0.0, "sam_perturb: eps = %g must be positive", eps);
  SamKeepTable tab;
  DTC_TRY(sam_keep_table("sam_perturb", keep, nkeep, true, &tab));
  const int64_t n4 = n / 4;
  const int nb = sam_norm_blocks(n);
  const dim3 grid(flat_blocks(n4, SAM_THREADS * SAM_UNROLL, SAM_MAX_BLOCKS));
  if (adaptive)
    DTC_KLAUNCH(sam_sumsq_kernel<true>, dim3(nb), dim3(SAM_NORM_THREADS), 0, st, g, p, n4, (double*)workspace, tab);
  else
    DTC_KLAUNCH(sam_sumsq_kernel<false>, dim3(nb), dim3(SAM_NORM_THREADS), 0, st, g, p, n4, (double*)workspace, tab);
  DTC_KLAUNCH(sam_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, nb, gmul, rho, eps,
              (SamState*)state);
  if (adaptive)
    DTC_KLAUNCH(sam_update_kernel<true>, grid, dim3(SAM_THREADS), 0, st, p, g, p_saved, p_bf16, n4,
                (const SamState*)state);
  else
    DTC_KLAUNCH(sam_update_kernel<false>, grid, dim3(SAM_THREADS), 0, st, p, g, p_saved, p_bf16, n4,
                (const SamState*)state);
  DTC_LAUNCH_CHECK();
  return 0;
}

int sam_restore(float* p, const float* p_saved, u16* p_bf16, int64_t n, const SamKeep* keep, int nkeep,
                const void* state, int* found_inf, hipStream_t st) {
  SAM_NONNULL("sam_restore", p);
  SAM_NONNULL("sam_restore", p_saved);
  SAM_NONNULL("sam_restore", p_bf16);
  SAM_NONNULL("sam_restore", state);
  DTC_TRY(sam_flat_args("sam_restore", p, p_saved, p_bf16, n));
  DTC_CHECK_ARG(aligned(state, 16), "sam_restore: state must be 16-byte aligned");
  SamKeepTable tab;
  DTC_TRY(sam_keep_table("sam_restore", keep, nkeep, false, &tab));
  const int64_t n4 = n / 4;
  DTC_KLAUNCH(sam_restore_kernel, dim3(flat_blocks(n4, SAM_THREADS * SAM_UNROLL, SAM_MAX_BLOCKS)), dim3(SAM_THREADS),
              0, st, p, p_saved, p_bf16, n4, (const SamState*)state, found_inf, tab);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
