// PowerSGD (Vogels, Karimireddy, Jaggi 2019, "PowerSGD: Practical Low-Rank Gradient Compression for Distributed
// Optimization"; torch's ddp_comm_hooks.powerSGD_hook) on the flat gradient buffer. A plan tells the device where
// every tensor lies and at which rank r (1..4; 0: uncompressed) it is compressed. Per step, with A = g + e (e: the
// error-feedback buffer, optional) and every compressed tensor seen as a row-major rows x cols matrix:
//   1. orthonormalize(Q):   Qh = MGS(Q), Q = the warm start chosen by the device word state[0]      one workgroup / tensor
//   2. project:             P = A Qh, and the uncompressed tensors packed in front of P: staging = [uncompressed | P]
//      -- the caller all-reduces staging --
//   3. orthonormalize(P):   Ph = MGS(P) in place; notes a non-finite P                               one workgroup / tensor
//   4. back-project:        Q = A^T Ph, the rows split over workgroups, one slot of doubles per row chunk, folded in
//                           index order by the chunk group's last workgroup
//      -- the caller all-reduces Q --
//   5. reconstruct:         gh = Ph Q^T -> g ;  e = (g + e) - c * gh ; the uncompressed tensors scattered back
// Five launches, no host synchronisation, no floating-point atomics: dot products are summed in double in a fixed
// order (per lane in index order, a butterfly over the wave, waves / slots in index order) and rounded to fp32 once,
// so every result is bit-identical from run to run. Elements between the tensors are neither read nor written.
//
// A non-finite all-reduced P or Q (the same verdict on every rank) makes step 5 write NaN into the compressed
// tensors' gradients and leave e alone. Q is kept twice: q[0] the warm start as it was before the step (step 1
// copies its source there), q[1] the working copy (Qh, then the new Q and its collective). Step 5 sets state[0] = 1
// (next source: q[1]) after a finite step and 0 (q[0]) otherwise; the host never reads it.
#include <new>
#include <vector>
#include "flat.h"
#include "kernels.h"

namespace dtc {

constexpr int PSGD_MAX_RANK = 4;
constexpr int PSGD_MAX_TENSORS = 4096;
constexpr int64_t PSGD_MAX_BLOCKS = 1 << 22;
constexpr int PSGD_THREADS = 256;
#ifndef DTC_PSGD_WAVE_ROWS  // (all three overridable at build time for A/B builds)
#define DTC_PSGD_WAVE_ROWS 2
#endif
#ifndef DTC_PSGD_BP_ROWS
#define DTC_PSGD_BP_ROWS 64
#endif
#ifndef DTC_PSGD_BP_UNROLL
#define DTC_PSGD_BP_UNROLL 4
#endif
constexpr int PSGD_WAVE_ROWS = DTC_PSGD_WAVE_ROWS;                  // rows of A per wave in project / reconstruct
constexpr int PSGD_WG_ROWS = PSGD_WAVE_ROWS * (PSGD_THREADS / 64);  // 8 rows per workgroup
constexpr int PSGD_FLAT_CHUNK = 4096;                               // uncompressed elements per workgroup
constexpr int PSGD_BP_ROWS = DTC_PSGD_BP_ROWS;                      // rows per back-project chunk
constexpr int PSGD_ORTH_THREADS = 1024;
constexpr int PSGD_ORTH_CAP = 5;  // rows a thread keeps in registers: 5 * 1024 covers ResNet-18's 4608 columns
constexpr double PSGD_DEPENDENT = 0x1p-40;  // (2^-20)^2: a column this close to the span of its predecessors is noise

struct PsgdTen {  // one tensor as the kernels read it (64 bytes)
  int64_t offset;    // in the flat buffers
  int64_t p_off;     // rank > 0: P block in staging; rank 0: its place in staging's head
  int64_t q_off;     // Q block
  int64_t slot_off;  // back-project partial slots (doubles)
  int32_t rows, cols, rank, nrc;  // rank 0: cols = 1 and rows*cols is kept in q_off; nrc: back-project row chunks
  int32_t tick0, comp;            // first arrival counter; index among the compressed tensors
  int32_t vecq, pad;              // 16-byte access to rows of A and to Q allowed
};
struct PsgdRowBlk {  // project / reconstruct work map
  int32_t ten, blk;
};
struct PsgdBpBlk {  // back-project work map
  int32_t ten, rc, cb, pad;
};

struct PsgdPlan {
  std::vector<PsgdTen> tens;
  std::vector<int32_t> comp;  // indices of the compressed tensors
  std::vector<PsgdRowBlk> rowmap;
  std::vector<PsgdBpBlk> bpmap;
  int64_t n_p = 0, n_q = 0, n_unc = 0, n_slots = 0;
  int32_t n_ticks = 0, first_comp_blk = -1;
  size_t off_comp = 0, off_rowmap = 0, off_bpmap = 0, off_slots = 0, off_ticks = 0, off_bad = 0, bytes = 0;
  void* dev = nullptr;
  const PsgdTen* d_tens() const { return (const PsgdTen*)dev; }
  const int32_t* d_comp() const { return (const int32_t*)((char*)dev + off_comp); }
  const PsgdRowBlk* d_rowmap() const { return (const PsgdRowBlk*)((char*)dev + off_rowmap); }
  const PsgdBpBlk* d_bpmap() const { return (const PsgdBpBlk*)((char*)dev + off_bpmap); }
  double* d_slots() const { return (double*)((char*)dev + off_slots); }
  unsigned* d_ticks() const { return (unsigned*)((char*)dev + off_ticks); }
  int* d_bad() const { return (int*)((char*)dev + off_bad); }
};

static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

int psgd_plan_create(PsgdPlan** out, const PsgdDesc* t, int n) {
  DTC_CHECK_ARG(out, "psgd_plan_create: null output pointer");
  *out = nullptr;
  DTC_CHECK_ARG(t, "psgd_plan_create: null tensor table");
  DTC_CHECK_ARG(n >= 1 && n <= PSGD_MAX_TENSORS, "psgd_plan_create: n = %d must lie in [1, %d]", n, PSGD_MAX_TENSORS);
  int64_t end = 0, blocks = 0;
  for (int i = 0; i < n; ++i) {
    const PsgdDesc& s = t[i];
    DTC_CHECK_ARG(s.rows >= 1 && s.cols >= 1, "psgd_plan_create: tensor %d: rows = %lld and cols = %lld must be positive",
                  i, (long long)s.rows, (long long)s.cols);
    DTC_CHECK_ARG(s.rows <= INT64_MAX / s.cols, "psgd_plan_create: tensor %d: rows * cols overflows", i);
    const int64_t numel = s.rows * s.cols;
    DTC_CHECK_ARG(s.offset >= 0 && s.offset % 4 == 0,
                  "psgd_plan_create: tensor %d: offset = %lld must be a non-negative multiple of 4", i,
                  (long long)s.offset);
    DTC_CHECK_ARG(numel <= INT64_MAX - s.offset, "psgd_plan_create: tensor %d: offset + rows * cols overflows", i);
    DTC_CHECK_ARG(s.offset >= end,
                  "psgd_plan_create: tensor %d (offset %lld) is not sorted after / overlaps its predecessor (end %lld)",
                  i, (long long)s.offset, (long long)end);
    DTC_CHECK_ARG(s.reserved == 0, "psgd_plan_create: tensor %d: reserved = %d must be 0", i, (int)s.reserved);
    DTC_CHECK_ARG(s.rank >= 0 && s.rank <= PSGD_MAX_RANK && s.rank <= s.rows && s.rank <= s.cols,
                  "psgd_plan_create: tensor %d: rank = %d must lie in [0, min(rows, cols, %d)]", i, (int)s.rank,
                  PSGD_MAX_RANK);
    DTC_CHECK_ARG(s.rank == 0 || (s.rows < (1ll << 31) && s.cols < (1ll << 31)),
                  "psgd_plan_create: tensor %d: a compressed tensor's rows and cols must be below 2^31", i);
    end = s.offset + numel;
    blocks += s.rank ? (s.rows - 1) / PSGD_WG_ROWS + 1 : (numel - 1) / PSGD_FLAT_CHUNK + 1;
    DTC_CHECK_ARG(blocks <= PSGD_MAX_BLOCKS, "psgd_plan_create: more than %lld workgroups of work",
                  (long long)PSGD_MAX_BLOCKS);
  }
  PsgdPlan* pl = new (std::nothrow) PsgdPlan;
  DTC_CHECK_ARG(pl, "psgd_plan_create: out of host memory");
  for (int i = 0; i < n; ++i)
    if (t[i].rank == 0) pl->n_unc += t[i].rows * t[i].cols;
  int64_t u = 0;
  for (int i = 0; i < n; ++i) {
    const PsgdDesc& s = t[i];
    PsgdTen d{};
    d.offset = s.offset;
    d.rank = s.rank;
    if (s.rank == 0) {
      const int64_t numel = s.rows * s.cols;
      d.p_off = u;
      d.q_off = numel;
      d.rows = d.cols = 1;
      d.comp = -1;
      u += numel;
      for (int64_t b = 0; b * PSGD_FLAT_CHUNK < numel; ++b) pl->rowmap.push_back(PsgdRowBlk{i, (int32_t)b});
    } else {
      d.rows = (int32_t)s.rows;
      d.cols = (int32_t)s.cols;
      d.p_off = pl->n_unc + pl->n_p;
      d.q_off = pl->n_q;
      d.vecq = (s.cols % 4 == 0 && pl->n_q % 4 == 0) ? 1 : 0;
      d.nrc = (int32_t)((s.rows - 1) / PSGD_BP_ROWS + 1);
      d.slot_off = pl->n_slots;
      d.tick0 = pl->n_ticks;
      d.comp = (int32_t)pl->comp.size();
      const int64_t percb = (int64_t)PSGD_THREADS * (s.cols % 4 == 0 ? 4 : 1);
      const int32_t ncb = (int32_t)((s.cols - 1) / percb + 1);
      if (d.nrc > 1) {
        pl->n_slots += (int64_t)d.nrc * s.cols * s.rank;
        pl->n_ticks += ncb;
      }
      if (pl->first_comp_blk < 0) pl->first_comp_blk = (int32_t)pl->rowmap.size();
      for (int64_t b = 0; b * PSGD_WG_ROWS < s.rows; ++b) pl->rowmap.push_back(PsgdRowBlk{i, (int32_t)b});
      for (int32_t rc = 0; rc < d.nrc; ++rc)
        for (int32_t cb = 0; cb < ncb; ++cb) pl->bpmap.push_back(PsgdBpBlk{i, rc, cb, 0});
      pl->comp.push_back(i);
      pl->n_p += s.rows * s.rank;
      pl->n_q += s.cols * s.rank;
    }
    pl->tens.push_back(d);
  }
  if ((int64_t)pl->bpmap.size() > PSGD_MAX_BLOCKS) {
    delete pl;
    return set_error(DTC_EINVAL, "psgd_plan_create: more than %lld workgroups of work", (long long)PSGD_MAX_BLOCKS);
  }
  pl->off_comp = up16(pl->tens.size() * sizeof(PsgdTen));
  pl->off_rowmap = up16(pl->off_comp + pl->comp.size() * sizeof(int32_t));
  pl->off_bpmap = up16(pl->off_rowmap + pl->rowmap.size() * sizeof(PsgdRowBlk));
  pl->off_slots = up16(pl->off_bpmap + pl->bpmap.size() * sizeof(PsgdBpBlk));
  pl->off_ticks = up16(pl->off_slots + (size_t)pl->n_slots * sizeof(double));
  pl->off_bad = up16(pl->off_ticks + (size_t)pl->n_ticks * sizeof(unsigned));
  pl->bytes = up16(pl->off_bad + (pl->comp.size() + 1) * sizeof(int));
  *out = pl;
  return 0;
}

int psgd_plan_destroy(PsgdPlan* plan) {
  delete plan;
  return 0;
}

int64_t psgd_plan_numel(const PsgdPlan* plan, int what) {
  if (!plan) return 0;
  switch (what) {
    case 0: return plan->n_p;
    case 1: return plan->n_q;
    case 2: return plan->n_unc;
    case 3: return plan->n_unc + plan->n_p;
    case 4: return (plan->n_q + 3) & ~(int64_t)3;
    default: return -1;
  }
}
size_t psgd_plan_device_bytes(const PsgdPlan* plan) { return plan ? plan->bytes : 0; }

int psgd_plan_bind(PsgdPlan* plan, void* dev, size_t bytes, hipStream_t st) {
  DTC_CHECK_ARG(plan && dev, "psgd_plan_bind: null pointer");
  DTC_CHECK_ARG(aligned(dev, 16), "psgd_plan_bind: the device region must be 16-byte aligned");
  DTC_CHECK_ARG(bytes >= plan->bytes, "psgd_plan_bind: %zu bytes given, the plan needs %zu", bytes, plan->bytes);
  plan->dev = nullptr;
  DTC_HIP(hipMemcpyAsync(dev, plan->tens.data(), plan->tens.size() * sizeof(PsgdTen), hipMemcpyHostToDevice, st));
  if (!plan->comp.empty())
    DTC_HIP(hipMemcpyAsync((char*)dev + plan->off_comp, plan->comp.data(), plan->comp.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, st));
  DTC_HIP(hipMemcpyAsync((char*)dev + plan->off_rowmap, plan->rowmap.data(), plan->rowmap.size() * sizeof(PsgdRowBlk),
                         hipMemcpyHostToDevice, st));
  if (!plan->bpmap.empty())
    DTC_HIP(hipMemcpyAsync((char*)dev + plan->off_bpmap, plan->bpmap.data(), plan->bpmap.size() * sizeof(PsgdBpBlk),
                           hipMemcpyHostToDevice, st));
  DTC_HIP(hipMemsetAsync((char*)dev + plan->off_ticks, 0, plan->bytes - plan->off_ticks, st));
  plan->dev = dev;
  return 0;
}

// ---------------------------------------------------------------- device helpers
// The sum of v over a workgroup of THREADS, the same bits in every thread: a butterfly over the wave, lane 0 of each
// wave to LDS, every thread adds the waves in index order. sh: THREADS / 64 doubles, free again on return.
template <int THREADS>
__device__ __forceinline__ double block_sum_all(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int w = 1; w < THREADS / 64; ++w) s += sh[w];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ f32x4 add4_rn(const f32x4& a, const f32x4& b) {
  return f32x4{__fadd_rn(a[0], b[0]), __fadd_rn(a[1], b[1]), __fadd_rn(a[2], b[2]), __fadd_rn(a[3], b[3])};
}

// ---------------------------------------------------------------- steps 1 and 3: modified Gram-Schmidt
// One workgroup per compressed tensor over its n x r block (row-major). A thread owns the rows t, t + THREADS, ...:
// it alone reads and writes them (the first PSGD_ORTH_CAP of them in registers), so only the sums synchronise. Column k: minus its projections on the finished
// columns one after the other, then divided by (norm + eps); norm + eps == 0 gives a zero column. A column whose
// norm fell to 2^-20 of what it was before the projections is divided by that earlier norm instead.
// IS_Q: src = state[0] ? q1 : q0, copied to q0 (the warm start as it was before this step), Qh to q1.
// !IS_Q: P in staging in place; bad[comp] = P holds a non-finite value; the tensor's arrival counters are zeroed.
template <bool IS_Q>
__global__ void __launch_bounds__(PSGD_ORTH_THREADS) psgd_orth_kernel(const PsgdTen* __restrict__ tens,
                                                                      const int32_t* __restrict__ comp, float* q0,
                                                                      float* q1, float* staging,
                                                                      const int* __restrict__ state, float eps,
                                                                      int* __restrict__ bad,
                                                                      unsigned* __restrict__ ticks) {
  constexpr int T = PSGD_ORTH_THREADS, CAP = PSGD_ORTH_CAP, R = PSGD_MAX_RANK;
  __shared__ double sh[T / 64];
  const PsgdTen tn = tens[comp[blockIdx.x]];
  const int r = tn.rank, t = threadIdx.x;
  const int n = IS_Q ? tn.cols : tn.rows;
  const bool from1 = IS_Q && state[0] != 0;
  const float* src = IS_Q ? (from1 ? q1 : q0) + tn.q_off : staging + tn.p_off;
  float* snap = IS_Q ? q0 + tn.q_off : nullptr;
  float* dst = IS_Q ? q1 + tn.q_off : staging + tn.p_off;
  // the thread's first CAP rows live in registers (absent rows and columns: zeros, which change no sum), any further
  // row stays in dst
  float v[CAP][R];
  int nf = 0;
#pragma unroll
  for (int u = 0; u < CAP; ++u) {
    const int i = t + u * T;
#pragma unroll
    for (int c = 0; c < R; ++c) {
      v[u][c] = (i < n && c < r) ? src[(int64_t)i * r + c] : 0.f;
      nf |= finite_f(v[u][c]) ? 0 : 1;
      if (from1 && i < n && c < r) snap[(int64_t)i * r + c] = v[u][c];
    }
  }
  for (int i = t + CAP * T; i < n; i += T)
    for (int c = 0; c < r; ++c) {
      const float x = src[(int64_t)i * r + c];
      nf |= finite_f(x) ? 0 : 1;
      if (from1) snap[(int64_t)i * r + c] = x;
      if (IS_Q) dst[(int64_t)i * r + c] = x;
    }
  if (!IS_Q) {
    nf = __syncthreads_or(nf);
    if (t == 0) bad[tn.comp] = nf;
    if (tn.nrc > 1) {
      const int64_t percb = (int64_t)PSGD_THREADS * (tn.cols % 4 == 0 ? 4 : 1);
      const int ncb = (int)((tn.cols - 1) / percb + 1);
      for (int i = t; i < ncb; i += T) ticks[tn.tick0 + i] = 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    if (k >= r) break;  // workgroup-uniform
    double proj2 = 0.0;  // what the projections took out of the column, squared
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (j >= k) break;
      double d = 0.0;
#pragma unroll
      for (int u = 0; u < CAP; ++u) d += (double)v[u][j] * (double)v[u][k];
      for (int i = t + CAP * T; i < n; i += T) d += (double)dst[(int64_t)i * r + j] * (double)dst[(int64_t)i * r + k];
      d = block_sum_all<T>(d, sh);
      proj2 += d * d;
#pragma unroll
      for (int u = 0; u < CAP; ++u) v[u][k] = (float)((double)v[u][k] - d * (double)v[u][j]);
      for (int i = t + CAP * T; i < n; i += T)
        dst[(int64_t)i * r + k] = (float)((double)dst[(int64_t)i * r + k] - d * (double)dst[(int64_t)i * r + j]);
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < CAP; ++u) s += (double)v[u][k] * (double)v[u][k];
    for (int i = t + CAP * T; i < n; i += T) {
      const double x = (double)dst[(int64_t)i * r + k];
      s += x * x;
    }
    s = block_sum_all<T>(s, sh);
    // a column that lay in the span of the finished ones leaves only rounding noise: divided by its own norm the
    // noise would become a unit vector that is not orthogonal to them. It is divided by the column's norm before
    // the projections instead (Pythagoras: the finished columns are orthonormal) and so stays negligible.
    const double before = s + proj2;
    const double den = sqrt(s <= PSGD_DEPENDENT * before ? before : s) + (double)eps;
#pragma unroll
    for (int u = 0; u < CAP; ++u) v[u][k] = den == 0.0 ? 0.f : (float)((double)v[u][k] / den);
    for (int i = t + CAP * T; i < n; i += T)
      dst[(int64_t)i * r + k] = den == 0.0 ? 0.f : (float)((double)dst[(int64_t)i * r + k] / den);
  }
#pragma unroll
  for (int u = 0; u < CAP; ++u) {
    const int i = t + u * T;
#pragma unroll
    for (int c = 0; c < R; ++c)
      if (i < n && c < r) dst[(int64_t)i * r + c] = v[u][c];
  }
}

// ---------------------------------------------------------------- shared by project and reconstruct
// the four columns 4 * jq .. + 3 of Q (cols x R, row-major) as 4 * R consecutive floats
template <int R>
struct QQuad {
  float v[4 * R];
};
template <int R>
__device__ __forceinline__ QQuad<R> load_qquad(const float* __restrict__ q, int jq) {
  QQuad<R> o;
  const f32x4* p = (const f32x4*)(q + (int64_t)jq * 4 * R);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const f32x4 x = p[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) o.v[4 * i + c] = x[c];
  }
  return o;
}

// ---------------------------------------------------------------- step 2: P = (g + e) Qh, uncompressed packed
template <int R>
__device__ __forceinline__ void project_rows(const PsgdTen& tn, int blk, const float* __restrict__ g,
                                             const float* __restrict__ e, const float* __restrict__ q,
                                             float* __restrict__ staging) {
  constexpr int WR = PSGD_WAVE_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blk * PSGD_WG_ROWS + wave * WR;
  if (row0 >= tn.rows) return;  // wave-uniform; no barrier follows
  const int nr = min(WR, tn.rows - row0);
  const int cols = tn.cols;
  const float* __restrict__ qh = q + tn.q_off;
  double acc[WR][R];
#pragma unroll
  for (int a = 0; a < WR; ++a)
#pragma unroll
    for (int k = 0; k < R; ++k) acc[a][k] = 0.0;
  if (tn.vecq) {
    for (int jq = lane; jq < cols / 4; jq += 64) {
      const QQuad<R> qq = load_qquad<R>(qh, jq);
#pragma unroll
      for (int a = 0; a < WR; ++a) {
        if (a < nr) {
          const int64_t o = tn.offset + (int64_t)(row0 + a) * cols + (int64_t)jq * 4;
          f32x4 x = *(const f32x4*)(g + o);
          if (e) x = add4_rn(x, *(const f32x4*)(e + o));
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < R; ++k) acc[a][k] += (double)x[c] * (double)qq.v[c * R + k];
        }
      }
    }
  } else {
    for (int j = lane; j < cols; j += 64) {
      float qv[R];
#pragma unroll
      for (int k = 0; k < R; ++k) qv[k] = qh[(int64_t)j * R + k];
#pragma unroll
      for (int a = 0; a < WR; ++a) {
        if (a < nr) {
          const int64_t o = tn.offset + (int64_t)(row0 + a) * cols + j;
          float x = g[o];
          if (e) x = __fadd_rn(x, e[o]);
#pragma unroll
          for (int k = 0; k < R; ++k) acc[a][k] += (double)x * (double)qv[k];
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < WR; ++a)
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const double s = wave_sum_d(acc[a][k]);
      if (lane == 0 && a < nr) staging[tn.p_off + (int64_t)(row0 + a) * R + k] = (float)s;
    }
}

__global__ void __launch_bounds__(PSGD_THREADS) psgd_project_kernel(const PsgdTen* __restrict__ tens,
                                                                    const PsgdRowBlk* __restrict__ map,
                                                                    const float* __restrict__ g,
                                                                    const float* __restrict__ e,
                                                                    const float* __restrict__ q,
                                                                    float* __restrict__ staging) {
  const PsgdRowBlk m = map[blockIdx.x];
  const PsgdTen tn = tens[m.ten];
  switch (tn.rank) {
    case 0: {
      const int64_t base = (int64_t)m.blk * PSGD_FLAT_CHUNK;
      const int len = (int)min((int64_t)PSGD_FLAT_CHUNK, tn.q_off - base);
      for (int i = threadIdx.x; i < len; i += PSGD_THREADS) staging[tn.p_off + base + i] = g[tn.offset + base + i];
      break;
    }
    case 1: project_rows<1>(tn, m.blk, g, e, q, staging); break;
    case 2: project_rows<2>(tn, m.blk, g, e, q, staging); break;
    case 3: project_rows<3>(tn, m.blk, g, e, q, staging); break;
    default: project_rows<4>(tn, m.blk, g, e, q, staging); break;
  }
}

// ---------------------------------------------------------------- step 4: Q = (g + e)^T Ph
// A workgroup takes PSGD_BP_ROWS rows of one column block: a thread owns V adjacent columns (V = 4 where rows of A
// are 16-byte aligned) and walks the rows in index order. One row chunk: the sums are Q. Several: each chunk writes
// its sums to its own slot; the chunk that arrives last at the column block's counter adds the slots in index order.
// Hand-off: plain slot stores, every wave drained, a workgroup barrier, lane 0 releases at agent scope and adds to
// the counter; the last arriver acquires at agent scope ahead of a barrier and the slot loads. No workgroup waits.
template <int R, int V>
__device__ __forceinline__ void backproject_block(const PsgdTen& tn, const PsgdBpBlk& m, const float* __restrict__ g,
                                                  const float* __restrict__ e, const float* __restrict__ staging,
                                                  float* __restrict__ q, double* __restrict__ slots,
                                                  unsigned* __restrict__ ticks, unsigned* lastflag) {
  const int cols = tn.cols;
  const int64_t j0 = ((int64_t)m.cb * PSGD_THREADS + threadIdx.x) * V;
  const bool active = j0 < cols;
  const int i0 = m.rc * PSGD_BP_ROWS, i1 = min(tn.rows, i0 + PSGD_BP_ROWS);
  const float* __restrict__ ph = staging + tn.p_off;
  double acc[V][R];
#pragma unroll
  for (int c = 0; c < V; ++c)
#pragma unroll
    for (int k = 0; k < R; ++k) acc[c][k] = 0.0;
  if (active) {
#pragma unroll DTC_PSGD_BP_UNROLL
    for (int i = i0; i < i1; ++i) {
      const int64_t o = tn.offset + (int64_t)i * cols + j0;
      float x[V];
      if (V == 4) {
        f32x4 xv = *(const f32x4*)(g + o);
        if (e) xv = add4_rn(xv, *(const f32x4*)(e + o));
#pragma unroll
        for (int c = 0; c < V; ++c) x[c] = xv[c];
      } else {
        x[0] = g[o];
        if (e) x[0] = __fadd_rn(x[0], e[o]);
      }
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const double p = (double)ph[(int64_t)i * R + k];
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c][k] += (double)x[c] * p;
      }
    }
  }
  float* __restrict__ qo = q + tn.q_off;
  if (tn.nrc == 1) {
    if (active) {
#pragma unroll
      for (int c = 0; c < V; ++c)
#pragma unroll
        for (int k = 0; k < R; ++k) qo[(j0 + c) * R + k] = (float)acc[c][k];
    }
    return;
  }
  double* __restrict__ sl = slots + tn.slot_off;
  const int64_t plane = (int64_t)cols * R;
  if (active) {
#pragma unroll
    for (int c = 0; c < V; ++c)
#pragma unroll
      for (int k = 0; k < R; ++k) sl[(int64_t)m.rc * plane + (j0 + c) * R + k] = acc[c][k];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old =
        __hip_atomic_fetch_add(ticks + tn.tick0 + m.cb, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned last = old == (unsigned)(tn.nrc - 1) ? 1u : 0u;
    if (last) {
      __hip_atomic_store(ticks + tn.tick0 + m.cb, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *(volatile unsigned*)lastflag = last;
  }
  __syncthreads();
  if (*(volatile unsigned*)lastflag == 0u || !active) return;  // no barrier follows
#pragma unroll
  for (int c = 0; c < V; ++c)
#pragma unroll
    for (int k = 0; k < R; ++k) acc[c][k] = 0.0;
  for (int rc = 0; rc < tn.nrc; ++rc) {
#pragma unroll
    for (int c = 0; c < V; ++c)
#pragma unroll
      for (int k = 0; k < R; ++k) acc[c][k] += sl[(int64_t)rc * plane + (j0 + c) * R + k];
  }
#pragma unroll
  for (int c = 0; c < V; ++c)
#pragma unroll
    for (int k = 0; k < R; ++k) qo[(j0 + c) * R + k] = (float)acc[c][k];
}

__global__ void __launch_bounds__(PSGD_THREADS) psgd_backproject_kernel(const PsgdTen* __restrict__ tens,
                                                                        const PsgdBpBlk* __restrict__ map,
                                                                        const float* __restrict__ g,
                                                                        const float* __restrict__ e,
                                                                        const float* __restrict__ staging,
                                                                        float* __restrict__ q,
                                                                        double* __restrict__ slots,
                                                                        unsigned* __restrict__ ticks) {
  __shared__ unsigned lastflag;
  const PsgdBpBlk m = map[blockIdx.x];
  const PsgdTen tn = tens[m.ten];
  const bool v4 = tn.cols % 4 == 0;
#define PSGD_BP(R)                                                                      \
  if (v4)                                                                               \
    backproject_block<R, 4>(tn, m, g, e, staging, q, slots, ticks, &lastflag);          \
  else                                                                                  \
    backproject_block<R, 1>(tn, m, g, e, staging, q, slots, ticks, &lastflag);          \
  break;
  switch (tn.rank) {
    case 1: PSGD_BP(1)
    case 2: PSGD_BP(2)
    case 3: PSGD_BP(3)
    default: PSGD_BP(4)
  }
#undef PSGD_BP
}

// ---------------------------------------------------------------- step 5: gh = Ph Q^T, the error, the scatter
template <int R>
__device__ __forceinline__ void reconstruct_rows(const PsgdTen& tn, int blk, float* __restrict__ g,
                                                 float* __restrict__ e, const float* __restrict__ staging,
                                                 const float* __restrict__ q, float c, bool bad) {
  constexpr int WR = PSGD_WAVE_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blk * PSGD_WG_ROWS + wave * WR;
  if (row0 >= tn.rows) return;
  const int nr = min(WR, tn.rows - row0);
  const int cols = tn.cols;
  const float nan = __uint_as_float(0x7fc00000u);
  if (bad) {  // e and the warm start stay as they were; GradScaler's check sees the NaN
    for (int a = 0; a < nr; ++a) {
      const int64_t o = tn.offset + (int64_t)(row0 + a) * cols;
      for (int j = lane; j < cols; j += 64) g[o + j] = nan;
    }
    return;
  }
  const float* __restrict__ qn = q + tn.q_off;
  double p[WR][R];
#pragma unroll
  for (int a = 0; a < WR; ++a)
#pragma unroll
    for (int k = 0; k < R; ++k) p[a][k] = a < nr ? (double)staging[tn.p_off + (int64_t)(row0 + a) * R + k] : 0.0;
  if (tn.vecq) {
    for (int jq = lane; jq < cols / 4; jq += 64) {
      const QQuad<R> qq = load_qquad<R>(qn, jq);
#pragma unroll
      for (int a = 0; a < WR; ++a) {
        if (a < nr) {
          const int64_t o = tn.offset + (int64_t)(row0 + a) * cols + (int64_t)jq * 4;
          f32x4 gh;
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < R; ++k) s += p[a][k] * (double)qq.v[cc * R + k];
            gh[cc] = (float)s;
          }
          if (e) {
            const f32x4 x = add4_rn(*(const f32x4*)(g + o), *(const f32x4*)(e + o));
            f32x4 en;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) en[cc] = __fsub_rn(x[cc], __fmul_rn(c, gh[cc]));
            *(f32x4*)(e + o) = en;
          }
          *(f32x4*)(g + o) = gh;
        }
      }
    }
  } else {
    for (int j = lane; j < cols; j += 64) {
      float qv[R];
#pragma unroll
      for (int k = 0; k < R; ++k) qv[k] = qn[(int64_t)j * R + k];
#pragma unroll
      for (int a = 0; a < WR; ++a) {
        if (a < nr) {
          const int64_t o = tn.offset + (int64_t)(row0 + a) * cols + j;
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < R; ++k) s += p[a][k] * (double)qv[k];
          const float gh = (float)s;
          if (e) e[o] = __fsub_rn(__fadd_rn(g[o], e[o]), __fmul_rn(c, gh));
          g[o] = gh;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(PSGD_THREADS) psgd_reconstruct_kernel(const PsgdTen* __restrict__ tens,
                                                                        const PsgdRowBlk* __restrict__ map,
                                                                        float* __restrict__ g, float* __restrict__ e,
                                                                        const float* __restrict__ staging,
                                                                        const float* __restrict__ q, int64_t n_q,
                                                                        const int* __restrict__ badp, int ncomp,
                                                                        int first_comp_blk, int* __restrict__ state,
                                                                        float c) {
  const PsgdRowBlk m = map[blockIdx.x];
  const PsgdTen tn = tens[m.ten];
  if (tn.rank == 0) {
    const int64_t base = (int64_t)m.blk * PSGD_FLAT_CHUNK;
    const int len = (int)min((int64_t)PSGD_FLAT_CHUNK, tn.q_off - base);
    for (int i = threadIdx.x; i < len; i += PSGD_THREADS) g[tn.offset + base + i] = staging[tn.p_off + base + i];
    return;
  }
  // the step's verdict, formed alike by every workgroup: a non-finite all-reduced P (noted by step 3) or Q
  int nf = 0;
  for (int i = threadIdx.x; i < ncomp; i += PSGD_THREADS) nf |= badp[i];
  const int64_t n4 = n_q >> 2;
  const f32x4* __restrict__ q4 = (const f32x4*)q;
  uint32_t ex = 0;  // a value is non-finite iff its exponent field is all ones
  for (int64_t i = threadIdx.x; i < n4; i += PSGD_THREADS) {
    const f32x4 v = q4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) ex |= ((__float_as_uint(v[k]) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
  }
  if (threadIdx.x < (int)(n_q & 3)) ex |= finite_f(q[4 * n4 + threadIdx.x]) ? 0u : 1u;
  const bool bad = __syncthreads_or(nf | (int)ex) != 0;
  if ((int)blockIdx.x == first_comp_blk && threadIdx.x == 0) {
    state[0] = bad ? 0 : 1;
    state[1] = bad ? 1 : 0;
  }
  switch (tn.rank) {
    case 1: reconstruct_rows<1>(tn, m.blk, g, e, staging, q, c, bad); break;
    case 2: reconstruct_rows<2>(tn, m.blk, g, e, staging, q, c, bad); break;
    case 3: reconstruct_rows<3>(tn, m.blk, g, e, staging, q, c, bad); break;
    default: reconstruct_rows<4>(tn, m.blk, g, e, staging, q, c, bad); break;
  }
}

// ---------------------------------------------------------------- launchers
static int64_t q_stride(const PsgdPlan* pl) { return (pl->n_q + 3) & ~(int64_t)3; }

// checked in this order by every phase: the plan, the pointers, then that the plan is bound
#define PSGD_BOUND(name) \
  DTC_CHECK_ARG(plan->dev, name ": the plan is not bound to device memory (dtc_psgd_plan_bind)")

int psgd_orthonormalize(PsgdPlan* plan, int what, float* q, float* staging, int* state, double eps, hipStream_t st) {
  DTC_CHECK_ARG(plan, "psgd_orthonormalize: null plan");
  DTC_CHECK_ARG(what == 0 || what == 1, "psgd_orthonormalize: what = %d must be 0 (P) or 1 (Q)", what);
  DTC_CHECK_ARG(eps >= 0.0, "psgd_orthonormalize: epsilon = %g must not be negative", eps);
  if (what == 1) {
    DTC_CHECK_ARG(q && state, "psgd_orthonormalize: null pointer (q, state)");
    DTC_CHECK_ARG(aligned(q, 16) && aligned(state, 16), "psgd_orthonormalize: q and state must be 16-byte aligned");
  } else {
    DTC_CHECK_ARG(staging, "psgd_orthonormalize: null pointer (staging)");
    DTC_CHECK_ARG(aligned(staging, 16), "psgd_orthonormalize: staging must be 16-byte aligned");
  }
  PSGD_BOUND("psgd_orthonormalize");
  if (plan->comp.empty()) return 0;
  const dim3 grid((unsigned)plan->comp.size());
  if (what == 1)
    DTC_KLAUNCH(psgd_orth_kernel<true>, grid, dim3(PSGD_ORTH_THREADS), 0, st, plan->d_tens(), plan->d_comp(), q,
                q + q_stride(plan), (float*)nullptr, (const int*)state, (float)eps, plan->d_bad(), plan->d_ticks());
  else
    DTC_KLAUNCH(psgd_orth_kernel<false>, grid, dim3(PSGD_ORTH_THREADS), 0, st, plan->d_tens(), plan->d_comp(),
                (float*)nullptr, (float*)nullptr, staging, (const int*)nullptr, (float)eps, plan->d_bad(),
                plan->d_ticks());
  DTC_LAUNCH_CHECK();
  return 0;
}

int psgd_project(PsgdPlan* plan, const float* g, const float* e, const float* q, float* staging, hipStream_t st) {
  DTC_CHECK_ARG(plan, "psgd_project: null plan");
  DTC_CHECK_ARG(g && q && staging, "psgd_project: null pointer");
  DTC_CHECK_ARG(aligned(g, 16) && aligned(e, 16) && aligned(q, 16) && aligned(staging, 16),
                "psgd_project: g, e, q and staging must be 16-byte aligned");
  PSGD_BOUND("psgd_project");
  DTC_KLAUNCH(psgd_project_kernel, dim3((unsigned)plan->rowmap.size()), dim3(PSGD_THREADS), 0, st, plan->d_tens(),
              plan->d_rowmap(), g, e, q + q_stride(plan), staging);
  DTC_LAUNCH_CHECK();
  return 0;
}

int psgd_backproject(PsgdPlan* plan, const float* g, const float* e, const float* staging, float* q, hipStream_t st) {
  DTC_CHECK_ARG(plan, "psgd_backproject: null plan");
  DTC_CHECK_ARG(g && q && staging, "psgd_backproject: null pointer");
  DTC_CHECK_ARG(aligned(g, 16) && aligned(e, 16) && aligned(q, 16) && aligned(staging, 16),
                "psgd_backproject: g, e, q and staging must be 16-byte aligned");
  PSGD_BOUND("psgd_backproject");
  if (plan->bpmap.empty()) return 0;
  DTC_KLAUNCH(psgd_backproject_kernel, dim3((unsigned)plan->bpmap.size()), dim3(PSGD_THREADS), 0, st, plan->d_tens(),
              plan->d_bpmap(), g, e, staging, q + q_stride(plan), plan->d_slots(), plan->d_ticks());
  DTC_LAUNCH_CHECK();
  return 0;
}

int psgd_reconstruct(PsgdPlan* plan, float* g, float* e, const float* staging, const float* q, int* state, double c,
                     hipStream_t st) {
  DTC_CHECK_ARG(plan, "psgd_reconstruct: null plan");
  DTC_CHECK_ARG(g && q && staging && state, "psgd_reconstruct: null pointer");
  DTC_CHECK_ARG(aligned(g, 16) && aligned(e, 16) && aligned(q, 16) && aligned(staging, 16) && aligned(state, 16),
                "psgd_reconstruct: g, e, q, staging and state must be 16-byte aligned");
  DTC_CHECK_ARG(c > 0.0 && c <= 1.0, "psgd_reconstruct: c = %g must lie in (0, 1] (1 / world size)", c);
  PSGD_BOUND("psgd_reconstruct");
  DTC_KLAUNCH(psgd_reconstruct_kernel, dim3((unsigned)plan->rowmap.size()), dim3(PSGD_THREADS), 0, st, plan->d_tens(),
              plan->d_rowmap(), g, e, staging, q + q_stride(plan), plan->n_q, (const int*)plan->d_bad(),
              (int)plan->comp.size(), plan->first_comp_blk, state, (float)c);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
