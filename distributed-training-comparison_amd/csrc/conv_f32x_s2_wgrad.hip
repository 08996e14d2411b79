// Split-bf16 weight gradients of a projection block of the fp32 executor, on the bf16 MFMA (v_mfma_f32_16x16x32_bf16)
// of gfx950: conv1's (3x3 / stride 2 / pad 1) and the 1x1 stride-2 shortcut's in ONE launch. fp32 NHWC x, fp32
// [N][H/2][W/2][K] dy (conv1's output gradient) and dsc (the shortcut's) in, fp32 dw [K][3][3][C] and dwsc [K][C] out,
// fp32-grade results.
//
//   dw  [k][r][s][c] = scale * sum over (n, p, q) of dy [n][p][q][k] * x[n][2p + r - 1][2q + s - 1][c]  (zero outside)
//   dwsc[k][c]       = scale * sum over (n, p, q) of dsc[n][p][q][k] * x[n][2p][2q][c]
//
// All three tensors are activations, so all three are split in the kernel (f32_split.h: a = a0 + a1 + a2, three bf16
// planes, once per loaded element), and a product is the six plane products of order i + j <= 2, smallest first, the
// (0,0) product last: conv_f32x_wgrad.hip's arithmetic. The shortcut is a tenth tap: the centre tap's x fragments
// against dsc instead of dy -- 64 more GEMM rows per tile, no second pass over x.
//
// Tile: a 512-thread workgroup owns the ten taps of a 64-input-channel slice against a 32-OUTPUT-channel slice,
// D[(tap, c)][k] (640 x 32 fp32), and reduces over 32-position steps of the [N][H/2][W/2] grid (whole output rows of
// one image, or whole 4x4 images). The 32-wide k slice is what makes the kernel fit: a 32-position step needs the
// column-split stride-2 halo of x (halo_box_col<2>, halo_tap_shift<2>, pitch 2 (wo + 1)): 170 / 162 / 180 halo rows
// for 16- / 8- / 4-wide output rows, 69,120 B of three 128-B-row planes, so with 64 output channels (24,576 B of dy +
// dsc) two stages exceed the CU's 160 KB and 640 x 64 accumulators in two sets are 160 registers a lane. With 32, dy
// and dsc share one 128-B row per position (16-B chunks 0-3 dy, 4-7 dsc), two stages fit, the accumulators are 80
// registers, and conv_f32x_wgrad.hip's one-barrier ring carries over; the price is that a c-slice's x halo is staged
// by K / 32 workgroups instead of K / 64 (they are neighbours in the grid and share it in L2).
// Steps are split across workgroups (split-K); each split writes an fp32 slab [split][K][10 C] (columns 9 C .. 10 C
// are the shortcut's) and conv_f32.hip's fixed-order f32_wgrad_reduce sums and scales it into dw and dwsc. One split
// writes scale * sum to dw / dwsc itself. No atomics: bit-identical run to run.
//
// Data movement per step: the x halo ((2 rows + 1) x (2 wo + 1) input pixels per image block x 64 channels) and the
// 32 x 32 dy and dsc tiles are fetched as fp32 with bounds-checked 16-B buffer loads into registers -- up to three
// (halo row, 8-channel) units per thread, and one dy unit (waves 4, 5) or dsc unit (waves 6, 7): 32 registers. Only
// the top row and the left column of the box can be padding (the extents are even; taps r = 2 / s = 2 read row H - 1 /
// column W - 1, real data); a padded pixel, an image past the batch and a position past the tensor (the ragged last
// step) are an offset outside the descriptor: zeros, no branch. The loads of step k + 1 are issued before the MFMAs
// of step k; after them every unit is split once (split8) and its three planes are written to the OTHER stage's LDS
// images (16-B chunk c of row r at chunk c ^ trswz(r)), and one barrier per step publishes them. Positions are the
// MFMA reduction index (one 32-deep k-step per step): fragments of both operands are read with ds_read_b64_tr_b16,
// the x halo shifted by halo_tap_shift<2>(tap) rows per tap.
// 8 waves: 4 along the 640 rows (10 fragments each) x 2 along the 32 output channels (1 fragment each). Rows 576 ..
// 639 (the shortcut) are fragments 6 .. 9 of the last wave row: every wave reads a second dy-side fragment for its
// fragments 6 .. 9, at a wave-uniform offset that is dsc's for that wave row and dy's for the others (no select).
// Fragments go in pairs so that consecutive MFMAs never share an accumulator; 60 MFMAs per wave and step. The x
// fragments' LDS offsets (20 registers) are computed once.
// Accumulators: two sets of 10 fragments. acc takes the (0,0) products, lo the five corrections (2^-8 of the sum and
// so 2^-8 of its roundings); they are added in the epilogue (conv_f32x_wgrad.hip's accumulation).
//
// LDS map (162,816 B of 163,840; one workgroup per CU), two stages of 81,408 B:
//   [0, 69120)       three x halo images (plane 0, 1, 2) of 180 rows x 128 B
//   [69120, 81408)   three dy | dsc images of 32 rows x 128 B (64 B of dy, 64 B of dsc per position)
// Registers: 208 of the 256 a wave has at 512 threads per workgroup (208 VGPR + 0 AGPR: 80 accumulators, 32 held
// operands, 36 plane fragments, 20 fragment offsets), 106 SGPR; no scratch (-Rpass-analysis=kernel-resource-usage).
// Measured worst |err| / conv2d_wgrad(|x|, |dy|) over the test shapes: 1.25e-7 (dw), 9.6e-8 (dwsc); the bound is
// 2^-22 = 2.38e-7. Measured speed: 1.3-2.6x the two conv_f32 weight gradients at batches
// 64 .. 256 of the model's three transition shapes; see conv_f32x_s2_wgrad_ok for where it is refused.
#include "common.h"
#include "f32_split.h"
#include "flat.h"
#include "kernels.h"
#include "tile_common.h"

namespace dtc {

constexpr int XS_HROWS = 180;
constexpr int XS_HPL = XS_HROWS * 128;           // one x halo image
constexpr int XS_DPL = 32 * 128;                 // one dy | dsc image
constexpr int XS_DY = 3 * XS_HPL;                // the dy | dsc images of a stage
constexpr int XS_STAGE = 3 * XS_HPL + 3 * XS_DPL;
constexpr int XS_UNITS = 3;                      // (halo row, 8-channel) units per thread and step: 3 x 512 >= 180 x 8
constexpr int XS_BK = 32;                        // output channels per tile
static_assert(2 * XS_STAGE <= 160 * 1024, "two stages in LDS");

struct XsParams {
  const float* x;    // NHWC fp32
  const float* dy;   // [N][Ho][Wo][K] fp32
  const float* dsc;  // [N][Ho][Wo][K] fp32
  float* out;        // slab [split][K][10 C], or dw with one split
  float* out_sc;     // the slab at column 9 C, or dwsc with one split
  int64_t split_stride;  // elements from one split's output to the next (one split: unused)
  int ld, ld_sc;     // row pitch of out / out_sc
  float scale;       // one split: scale; slabs: 1
  int N, H, W, C, K, Ho, Wo;
  uint32_t x_bytes, dy_bytes;
  int rows, imgs, hb, nh;  // output rows / images per step, halo rows per image block and per step
  int spimg;               // steps per image (imgs == 1)
  int nsteps, steps_per_split;
  u64* ts;
};


__global__ void __launch_bounds__(512) conv_f32x_s2_wgrad_kernel(const XsParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * XS_STAGE];
  stamp_start(p.ts);
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ktiles = p.K / XS_BK;
  const int tile = blockIdx.x, split = blockIdx.y;
  const int c0 = (tile / ktiles) * 64, k0 = (tile % ktiles) * XS_BK;
  const int st_begin = split * p.steps_per_split;
  const int st_end = min(p.nsteps, st_begin + p.steps_per_split);
  const int hwh = p.Wo + 1, pitch = 2 * hwh, pc = t & 7;
  const int M = p.N * p.Ho * p.Wo;

  // ---- loads: unit u of this thread is halo row (u 512 + t) / 8, channels c0 + 8 pc .. + 7, relative to the step's
  // first input row; waves 4 .. 7: one (position, 8-channel) unit of dy (waves 4, 5) or dsc (6, 7)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rd =
      __builtin_amdgcn_make_buffer_rsrc((void*)(wave >= 6 ? p.dsc : p.dy), 0, p.dy_bytes, 0x00020000);
  int hrel[XS_UNITS], hyi[XS_UNITS];  // byte offset from the step's first input row; (image << 16) | box row, -1: never
#pragma unroll
  for (int u = 0; u < XS_UNITS; ++u) {
    const int hr = (u * 512 + t) >> 3;
    hrel[u] = 0;
    hyi[u] = -1;
    if (hr < p.nh) {
      const int i = hr / p.hb, rem = hr - i * p.hb;
      const int by = rem / pitch, hx = rem - by * pitch;
      const int col = halo_box_col<2>(hx, hwh);  // box column: input column col - 1
      if (col >= 1) {                            // (col - 1 <= 2 wo - 1 = W - 1: only the left column is padding)
        hrel[u] = (((i * p.H + by - 1) * p.W + col - 1) * p.C + c0 + pc * 8) * 4;
        hyi[u] = (i << 16) | by;
      }
    }
  }
  const int dt = t & 127, drow = dt >> 2, dch = dt & 3;   // waves 4 .. 7: position of the step, 16-B chunk of 32 k
  const int dchunk = (wave >= 6 ? 4 : 0) + dch;           // its chunk of the shared dy | dsc row
  const uint32_t drel = (uint32_t)((drow * p.K + k0 + dch * 8) * 4);
  f32x4 pf[XS_UNITS + 1][2];  // the next step's operands, fp32, in flight / held until the step boundary
  auto load_step = [&](int step) {
    int n0, y0;  // first image and first output row of the step
    if (p.imgs == 1) {
      n0 = step / p.spimg;
      y0 = (step - n0 * p.spimg) * p.rows;
    } else {
      n0 = step * p.imgs;
      y0 = 0;
    }
    const int base = ((n0 * p.H + 2 * y0) * p.W) * p.C * 4;
#pragma unroll
    for (int u = 0; u < XS_UNITS; ++u) {
      if (u == XS_UNITS - 1 && wave >= 7) break;  // rows 128 .. 179: waves 0 .. 6
      const int i = hyi[u] >> 16, y = 2 * y0 + (hyi[u] & 0xffff) - 1;  // y <= H - 1; -1: the top padding
      const bool ok = hyi[u] >= 0 && n0 + i < p.N && y >= 0;
      f32x_load16(rx, ok ? (uint32_t)(base + hrel[u]) : DMA_OOB, pf[u]);
    }
    if (wave >= 4) {
      const int m = step * 32 + drow;
      f32x_load16(rd, m < M ? (uint32_t)(step * 32 * p.K * 4) + drel : DMA_OOB, pf[XS_UNITS]);
    }
  };
  auto write_step = [&](char* sb) {  // split the held step and write its six images
#pragma unroll
    for (int u = 0; u < XS_UNITS; ++u) {
      if (u == XS_UNITS - 1 && wave >= 7) break;
      const int hr = (u * 512 + t) >> 3;
      if (u < XS_UNITS - 1 || hr < XS_HROWS) f32x_split_write(pf[u], sb + hr * 128 + ((pc ^ trswz(hr)) << 4), XS_HPL);
    }
    if (wave >= 4) f32x_split_write(pf[XS_UNITS], sb + XS_DY + drow * 128 + ((dchunk ^ trswz(drow)) << 4), XS_DPL);
  };

  // ---- fragments. Lane (lg, lq, lp) of a tr read h addresses position 8 lg + lq + 4 h of the step, 8-B unit
  // (fragment's first channel / 4) + lp of its row
  const int li = lane & 15, lq = li >> 2, lp = li & 3, lg = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;  // wave row (160 of the 640 GEMM rows) and column half (16 output channels)
  int hm[2];                                // halo row, at tap (0, 0), of the two positions
  uint32_t b0[2], b1[2];                    // dy fragment; fragments 6 .. 9's: dsc for the last wave row, else dy again
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int tp = 8 * lg + lq + 4 * h;
    const int spi = p.rows * p.Wo;  // positions per image block of a step
    const int ii = tp / spi, rem = tp - ii * spi;
    const int pr = rem / p.Wo, q = rem - pr * p.Wo;
    hm[h] = ii * p.hb + 2 * pr * pitch + q;
    b0[h] = (uint32_t)(XS_DY + tp * 128 + (((wn * 4 + lp) ^ f32x_uswz(tp)) << 3));
    b1[h] = (uint32_t)(XS_DY + tp * 128 + ((((wm == 3 ? 8 : 0) + wn * 4 + lp) ^ f32x_uswz(tp)) << 3));
  }
  uint32_t ao[10][2];  // x fragment i: GEMM row = tap 64 + channel; tap 9 (the shortcut) reads the centre tap
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int row = wm * 160 + i * 16;
    const int tap = row >> 6, unit = ((row & 63) >> 2) + lp;
    const int toff = halo_tap_shift<2>(tap == 9 ? 4 : tap, pitch, hwh);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ra = hm[h] + toff;
      ao[i][h] = (uint32_t)(ra * 128 + ((unit ^ f32x_uswz(ra)) << 3));
    }
  }

  f32x4 acc[10], lo[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) acc[i] = lo[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const char* sb) {
    bf16x8 bd[2][3];  // [0]: fragments 0 .. 5, [1]: fragments 6 .. 9
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      bd[0][pl] = f32x_tr8(sb + pl * XS_DPL, b0[0], b0[1]);
      bd[1][pl] = f32x_tr8(sb + pl * XS_DPL, b1[0], b1[1]);
    }
#pragma unroll
    for (int i = 0; i < 10; i += 2) {
      bf16x8 ax[2][3];
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) ax[e][pl] = f32x_tr8(sb + pl * XS_HPL, ao[i + e][0], ao[i + e][1]);
      const bf16x8(&b)[3] = bd[i >= 6];
      constexpr int PX[6] = {2, 1, 0, 1, 0, 0}, PD[6] = {0, 1, 2, 0, 1, 0};  // (x plane, dy plane)
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          if (q < 5) lo[i + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[e][PX[q]], b[PD[q]], lo[i + e], 0, 0, 0);
          else acc[i + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[e][0], b[0], acc[i + e], 0, 0, 0);
    }
  };

  // ---- step loop over two LDS stages. Step k: issue the loads of step k + 1 (registers), compute stage k & 1,
  // split and write step k + 1 into the other stage, barrier: every wave has written its share of step k + 1 and
  // is done reading step k, whose stage the step after next overwrites.
  if (st_begin < st_end) {
    load_step(st_begin);
    write_step(smem);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    for (int k = st_begin; k < st_end; ++k) {
      char* const sb = smem + ((k - st_begin) & 1) * XS_STAGE;
      char* const nb = smem + ((k - st_begin + 1) & 1) * XS_STAGE;
      const bool more = k + 1 < st_end;
      if (more) load_step(k + 1);
      __builtin_amdgcn_sched_barrier(0);
      compute(sb);
      __builtin_amdgcn_sched_barrier(0);
      if (more) write_step(nb);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }

  // ---- epilogue: out[k][tap C + c0 + c] / out_sc[k][c0 + c] (4 consecutive c per lane: one 16-B store)
  float* const out = p.out + (size_t)split * p.split_stride;
  float* const out_sc = p.out_sc + (size_t)split * p.split_stride;
  const int kout = k0 + wn * 16 + li;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int row = wm * 160 + i * 16 + 4 * lg;
    const int tap = row >> 6, c = c0 + (row & 63);
    float* const dst = tap == 9 ? out_sc + (size_t)kout * p.ld_sc + c : out + (size_t)kout * p.ld + tap * p.C + c;
    *(f32x4*)dst = (acc[i] + lo[i]) * p.scale;
  }
  stamp_end(p.ts);
}

// ---------------------------------------------------------------- host side
struct XsGeom {
  int rows = 0, imgs = 0, hb = 0, nh = 0, nsteps = 0;
};
// Step geometry of a feasible shape: 32 positions of the [H/2][W/2] grid are whole rows of one image or whole images
// (a last step of fewer images than `imgs` is padded with zeros by the loads)
static bool xs_geometry(const ConvShape& s, XsGeom& g) {
  if (!conv3x3_ok(s, 2) || s.H % 2 || s.W % 2) return false;
  const int ho = s.H / 2, wo = s.W / 2;
  if (wo != 4 && wo != 8 && wo != 16) return false;
  TileSplit t;
  if (!classic_tile(ho, wo, 32, t)) return false;
  g.rows = t.rows;
  g.imgs = t.imgs;
  g.hb = (2 * t.rows + 1) * 2 * (wo + 1);
  g.nh = t.imgs * g.hb;
  // 32-bit byte offsets of the fp32 tensors (the buffer descriptors' range; DMA_OOB must lie outside it)
  if (g.nh > XS_HROWS || (uint64_t)s.N * s.H * s.W * s.C * 4 >= (1ull << 31) ||
      (uint64_t)s.N * ho * wo * s.K * 4 >= (1ull << 31))
    return false;
  g.nsteps = t.imgs == 1 ? s.N * (ho / t.rows) : (s.N + t.imgs - 1) / t.imgs;
  return true;
}

// Every feasible geometry but the small 16-wide-row problems: measured against the two conv_f32 weight gradients at
// batches 32 / 64 / 128 / 256 of the model's three shapes the fused launch is 1.27-2.57x faster, the
// ranges of five rounds disjoint, except layer 2 at batch 32 (0.99x: 64 splits of 4 steps write and reduce a 21 MB
// slab for 2.7 GFLOP). Work in (step, tile) units: 16-wide rows lost at 1024 units and won from 2048 on, so fewer
// than 2048 are refused there; 8- and 4-wide rows won at every measured size (1024 units the smallest). Other channel
// counts of a row width are taken at equal units: extrapolated, not measured
bool conv_f32x_s2_wgrad_ok(const ConvShape& s) {
  XsGeom g;
  if (!xs_geometry(s, g)) return false;
  if (option_get(OPT_F32X_S2_WGRAD) >= 2) return true;  // every feasible geometry: for measuring the refused ones
  return s.W / 2 != 16 || (int64_t)g.nsteps * (s.C / 64) * (s.K / XS_BK) >= 2048;
}

size_t conv_f32x_s2_wgrad_workspace(const ConvShape& s) {
  XsGeom g;
  if (!xs_geometry(s, g)) return 0;
  const size_t one = (size_t)s.K * 10 * s.C * 4;
  const int splits = f32x_wgrad_splits_on_hand((s.C / 64) * (s.K / XS_BK), g.nsteps, one, SIZE_MAX);
  return splits == 1 ? 0 : splits * one;
}

int conv_f32x_s2_wgrad(const ConvShape& s, const float* x, const float* dy, const float* dsc, float* dw, float* dwsc,
                       float scale, float* slab, size_t slab_bytes, hipStream_t st, u64* ts) {
  XsGeom g;
  DTC_CHECK_ARG(xs_geometry(s, g), "conv_f32x_s2_wgrad: unsupported shape");
  DTC_CHECK_ARG(x && dy && dsc && dw && dwsc && aligned(x, 16) && aligned(dy, 16) && aligned(dsc, 16) &&
                    aligned(dw, 16) && aligned(dwsc, 16) && (!slab || aligned(slab, 16)),
                "conv_f32x_s2_wgrad: null / misaligned argument");
  const int C10 = 10 * s.C, tiles = (s.C / 64) * (s.K / XS_BK);
  const int splits = f32x_wgrad_splits_on_hand(tiles, g.nsteps, (size_t)s.K * C10 * 4, slab ? slab_bytes : 0);
  XsParams p{};
  p.x = x; p.dy = dy; p.dsc = dsc;
  if (splits == 1) {
    p.out = dw; p.ld = 9 * s.C;
    p.out_sc = dwsc; p.ld_sc = s.C;
    p.scale = scale;
  } else {
    p.out = slab; p.out_sc = slab + 9 * s.C;
    p.ld = p.ld_sc = C10;
    p.split_stride = (int64_t)s.K * C10;
    p.scale = 1.f;
  }
  p.N = s.N; p.H = s.H; p.W = s.W; p.C = s.C; p.K = s.K;
  p.Ho = s.H / 2; p.Wo = s.W / 2;
  p.x_bytes = (uint32_t)((uint64_t)s.N * s.H * s.W * s.C * 4);
  p.dy_bytes = (uint32_t)((uint64_t)s.N * p.Ho * p.Wo * s.K * 4);
  p.rows = g.rows; p.imgs = g.imgs; p.hb = g.hb; p.nh = g.nh;
  p.spimg = p.Ho / g.rows;
  p.nsteps = g.nsteps;
  p.steps_per_split = (g.nsteps + splits - 1) / splits;
  p.ts = ts;
  const dim3 grid((unsigned)tiles, (unsigned)splits);
  DTC_KLAUNCH(conv_f32x_s2_wgrad_kernel, grid, dim3(512), 0, st, p);
  DTC_LAUNCH_CHECK();
  if (splits == 1) return 0;
  DTC_TRY(f32_wgrad_reduce(slab, splits, s.K, C10, 9 * s.C, 9 * s.C, scale, dw, st, ts));
  return f32_wgrad_reduce(slab + 9 * s.C, splits, s.K, C10, s.C, s.C, scale, dwsc, st, ts);
}

}  // namespace dtc
