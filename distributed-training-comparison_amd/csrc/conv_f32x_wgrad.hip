// Split-bf16 weight gradient of the 3x3 / stride 1 / pad 1 convolutions of the fp32 executor, on the bf16 MFMA
// (v_mfma_f32_16x16x32_bf16) of gfx950: fp32 NHWC x and fp32 NPQK dy in, fp32 KRSC dw out, fp32-grade results.
//
//   dw[k][r][s][c] = scale * sum over (n, y, x) of dy[n][y][x][k] * xin[n][y + r - 1][x + s - 1][c]
//
// Both operands are activations, so both are split in the kernel (f32_split.h: a = a0 + a1 + a2, three bf16 planes)
// and the product is the six plane products of order i + j <= 2, as in conv_f32x.hip. The work split is
// wgrad_halo.hip's: a 512-thread workgroup owns all nine taps of a 64-input-channel slice against a 64-output-
// channel slice, D[(r, s, c)][k] (576 x 64 fp32), and reduces over 64-pixel steps (whole rows of one image, or whole
// 8x8 / 4x4 images); the steps are split across workgroups, each split writes an fp32 slab [split][K][9 C], and
// conv_f32.hip's fixed-order f32_wgrad_reduce sums and scales them. One split writes scale * sum to dw itself.
// No atomics: bit-identical run to run. Pixels past the tensor (a ragged last step) load zeros of both operands.
//
// Data movement per step: the zero-padded x halo ((rows + 2) x (W + 2) pixels x 64 channels, at most 144 halo rows)
// and the 64 x 64 dy tile are fetched as fp32 with 16-B buffer loads into registers -- three (halo row, 8-channel)
// units and one dy unit per thread, 32 registers; a padded or out-of-range pixel is an offset outside the
// descriptor: zeros, no branch. The loads of step k + 1 are issued before the MFMAs of step k; after them every unit
// is split once (split8) and its three planes are written to the OTHER stage's LDS images (128-B rows of 64
// channels, 16-B chunk c of row r at chunk c ^ trswz(r): a function of the row, so all nine shifted tap windows
// stay conflict-free), and one barrier per step publishes them. Pixels are the MFMA reduction index: fragments of
// both operands are read with ds_read_b64_tr_b16, the x halo shifted by r (W + 2) + s rows per tap.
// 8 waves: 4 along the 576 rows (9 fragments each) x 2 along the 64 output channels (2 fragments each). Per 32-pixel
// k-step and x fragment: 3 + 3 plane fragments, then the six products smallest first, (0,0) last, the two dy
// fragments alternating so consecutive MFMAs never share an accumulator; 216 MFMAs per wave and step.
// Accumulators: two sets of 18 fragments. acc takes the (0,0) products, lo the five corrections (2^-8 of the sum and
// so 2^-8 of its roundings); they are added in the epilogue. The pixel reduction of one workgroup is a few
// thousand pixels at most (the splits fill the chip), so there is no third set for periodic VALU sums.
// Registers: the per-fragment LDS offsets of the x halo (36 in wgrad_halo.hip) are recomputed from four per-lane halo
// rows in every step -- about 300 VALU instructions beside 216 MFMAs -- because 144 accumulator registers leave no
// room to keep them; the four rows pass through an empty asm in the step loop so that the compiler does not hoist
// the offsets back out of it.
//
// LDS map (159,744 B of 163,840; one workgroup per CU), two stages of 79,872 B:
//   [0, 55296)       three x halo images (plane 0, 1, 2) of 144 rows x 128 B
//   [55296, 79872)   three dy images of 64 rows x 128 B
// Registers: 254 of the 256 a wave has at 512 threads per workgroup (254 VGPR + 0 AGPR: 144 accumulators, 32 held
// operands, 36 plane fragments), 92 SGPR; no scratch. Two LDS stages because the registers hold one step of operands.
// Measured: 1.8-2.9x conv_f32's weight gradient at batch 256, 1.1-1.2x at batch 32.
// Two instances (-Rpass-analysis=kernel-resource-usage): the classic one above (GEN = 0: 254 VGPR + 0 AGPR, 92 SGPR, no
// scratch) and the general geometry's (GEN = 1, at the kernel: 252 VGPR + 0 AGPR, 106 SGPR, no scratch; the same LDS
// map), measured 2.0-3.3x conv_f32's weight gradient at rows of 224 / 112 / 56 / 28 / 14 / 7.
#include "common.h"
#include "f32_split.h"
#include "flat.h"
#include "kernels.h"
#include "tile_common.h"

namespace dtc {

constexpr int XW_HROWS = 144;
constexpr int XW_HPL = XW_HROWS * 128;           // one x halo image
constexpr int XW_DPL = 64 * 128;                 // one dy image
constexpr int XW_DY = 3 * XW_HPL;                // the dy images of a stage
constexpr int XW_STAGE = 3 * XW_HPL + 3 * XW_DPL;
constexpr int XW_UNITS = 3;                      // (halo row, 8-channel) units per thread and step: 3 x 512 >= 144 x 8
static_assert(2 * XW_STAGE <= 160 * 1024, "two stages in LDS");

struct XwParams {
  const float* x;   // NHWC fp32
  const float* dy;  // NPQK fp32 (stride 1, pad 1: P = H, Q = W)
  float* out;       // slab [split][K][9 C], or dw with one split
  float scale;      // one split: dw = scale * sum; slabs: 1
  int N, H, W, C, K;
  uint32_t x_bytes, dy_bytes;
  int rows, imgs, hb, nh;  // output rows / images per step, halo rows per image block and per step
  int spimg;               // steps per image (imgs == 1)
  int nsteps, steps_per_split;
  u64* ts;
  // general geometry (GEN): a step is `rows` rows x one seg-column segment of one image, spr segments per row, tpi
  // steps per image; x_bytes / dy_bytes are ONE image (the descriptors are made per step)
  int seg, spr, tpi;
  FastDiv fd_tpi, fd_spr;
};

// pixel (within the 64-pixel step) of k-step ks, lane block b = lane >> 4, tr read h, lane quad q
__device__ __forceinline__ int xw_pixel(int ks, int b, int h, int q) { return ks * 32 + 8 * b + q + 4 * h; }

// GEN = 1, the general (row segment) geometry of tile_common.h, for rows the classic step does not cover (224 / 112 /
// 56 / 28 / 14 / 7 wide) and tensors past 2 GiB: a step is rs rows x one seg-column segment of ONE image (the pair is
// xw_geometry_gen's choice), origin (n0, y0, q0) from seg_tile_origin, wave-uniform. Halo: the (rs + 2) x (seg + 2) box
// around it at pitch seg + 2; halo column hx is image column q0 + hx - 1, row hy image row y0 + hy - 1, real data wherever
// that lies inside the image (a neighbouring segment's or step's pixels) and an offset outside the descriptor only
// where it leaves the image. Slots: l of 64 is row l / seg, column l % seg of the step, dense; a slot at or past
// rs seg loads zeros of dy, so whatever halo rows its tr reads address (inside the 144 rows for every tap:
// xw_geometry_gen checks it; all 144 are written every step) it adds exactly nothing. Addressing: both buffer
// descriptors are made per step over the step's image (base x + n0 H W C, dy + n0 H W K in 64-bit arithmetic, range
// one image) and live in SGPRs for the loads of that step only; every in-kernel offset stays 32-bit, so the tensors
// may pass 2 GiB. imgs == 1, so hyi packs (halo column << 16) | halo row. Everything else is the classic kernel.
template <int GEN>
__global__ void __launch_bounds__(512) conv_f32x_wgrad_kernel(const XwParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * XW_STAGE];
  stamp_start(p.ts);
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ktiles = p.K >> 6;
  const int tile = blockIdx.x, split = blockIdx.y;
  const int c0 = (tile / ktiles) * 64, k0 = (tile % ktiles) * 64;
  const int st_begin = split * p.steps_per_split;
  const int st_end = min(p.nsteps, st_begin + p.steps_per_split);
  const int W2 = (GEN ? p.seg : p.W) + 2, pc = t & 7;
  const int M = p.N * p.H * p.W;

  // ---- loads: unit u of this thread is halo row (u 512 + t) / 8, channels c0 + 8 pc .. + 7, relative to the step's
  // first pixel; the dy unit is pixel t / 8 of the step, channels k0 + 8 pc .. + 7
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, p.dy_bytes, 0x00020000);
  // byte offset from the step's first pixel; (image << 16) | (row + 1) [GEN: (column + 1) << 16 | (row + 1)], -1: never
  int hrel[XW_UNITS], hyi[XW_UNITS];
#pragma unroll
  for (int u = 0; u < XW_UNITS; ++u) {
    const int hr = (u * 512 + t) >> 3;
    hrel[u] = 0;
    hyi[u] = -1;
    if (GEN && hr < p.nh) {
      const int hy = hr / W2, hx = hr - hy * W2;
      hrel[u] = (((hy - 1) * p.W + hx - 1) * p.C + c0 + pc * 8) * 4;
      hyi[u] = (hx << 16) | hy;
    } else if (hr < p.nh) {
      const int i = hr / p.hb, rem = hr - i * p.hb;
      const int hy = rem / W2, hx = rem - hy * W2;
      if ((unsigned)(hx - 1) < (unsigned)p.W) {
        hrel[u] = (((i * p.H + hy - 1) * p.W + hx - 1) * p.C + c0 + pc * 8) * 4;
        hyi[u] = (i << 16) | hy;
      }
    }
  }
  const int drow = t >> 3;
  uint32_t drel = (uint32_t)((drow * p.K + k0 + pc * 8) * 4);
  if constexpr (GEN) {  // slot drow is pixel (drow / seg, drow % seg) of the step; a padded slot loads zeros
    const int dr = drow / p.seg;
    drel = dr < p.rows ? (uint32_t)(((dr * p.W + drow - dr * p.seg) * p.K + k0 + pc * 8) * 4) : DMA_OOB;
  }
  f32x4 pf[XW_UNITS + 1][2];  // the next step's operands, fp32, in flight / held until the step boundary
  auto load_step = [&](int step) {
    if constexpr (GEN) {
      int n0, y0, q0;
      seg_tile_origin(step, p.tpi, p.fd_tpi, p.spr, p.fd_spr, p.rows, p.seg, n0, y0, q0);
      n0 = __builtin_amdgcn_readfirstlane(n0);  // (the descriptors are per step: keep them in SGPRs)
      y0 = __builtin_amdgcn_readfirstlane(y0);
      q0 = __builtin_amdgcn_readfirstlane(q0);
      const size_t img = (size_t)n0 * p.H * p.W;
      const auto gx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + img * p.C), 0, p.x_bytes, 0x00020000);
      const auto gd = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dy + img * p.K), 0, p.dy_bytes, 0x00020000);
      const uint32_t pix0 = (uint32_t)(y0 * p.W + q0);
#pragma unroll
      for (int u = 0; u < XW_UNITS; ++u) {
        if (u == XW_UNITS - 1 && wave >= 2) break;  // rows 128 .. 143: waves 0 and 1
        const int y = y0 + (hyi[u] & 0xffff) - 1, xc = q0 + (hyi[u] >> 16) - 1;
        const bool ok = hyi[u] >= 0 && (unsigned)y < (unsigned)p.H && (unsigned)xc < (unsigned)p.W;
        f32x_load16(gx, ok ? pix0 * (uint32_t)(p.C * 4) + (uint32_t)hrel[u] : DMA_OOB, pf[u]);
      }
      f32x_load16(gd, drel != DMA_OOB ? pix0 * (uint32_t)(p.K * 4) + drel : DMA_OOB, pf[XW_UNITS]);
      return;
    }
    int n0, y0;
    if (p.imgs == 1) {
      n0 = step / p.spimg;
      y0 = (step - n0 * p.spimg) * p.rows;
    } else {
      n0 = step * p.imgs;
      y0 = 0;
    }
    const int base = ((n0 * p.H + y0) * p.W) * p.C * 4;
#pragma unroll
    for (int u = 0; u < XW_UNITS; ++u) {
      if (u == XW_UNITS - 1 && wave >= 2) break;  // rows 128 .. 143: waves 0 and 1
      const int i = hyi[u] >> 16, y = y0 + (hyi[u] & 0xffff) - 1;
      const bool ok = hyi[u] >= 0 && n0 + i < p.N && (unsigned)y < (unsigned)p.H;
      f32x_load16(rx, ok ? (uint32_t)(base + hrel[u]) : DMA_OOB, pf[u]);
    }
    const int m = step * 64 + drow;
    f32x_load16(rd, m < M ? (uint32_t)(step * 64 * p.K * 4) + drel : DMA_OOB, pf[XW_UNITS]);
  };
  auto write_step = [&](char* sb) {  // split the held step and write its six images
#pragma unroll
    for (int u = 0; u < XW_UNITS; ++u) {
      if (u == XW_UNITS - 1 && wave >= 2) break;
      const int hr = (u * 512 + t) >> 3;
      f32x_split_write(pf[u], sb + hr * 128 + ((pc ^ trswz(hr)) << 4), XW_HPL);
    }
    f32x_split_write(pf[XW_UNITS], sb + XW_DY + drow * 128 + ((pc ^ trswz(drow)) << 4), XW_DPL);
  };

  // ---- per-lane halo row, at tap (0, 0), of the pixels this lane's tr reads address
  const int li = lane & 15, lq = li >> 2, lp = li & 3, lg = lane >> 4;
  const int spi = p.rows * p.W;  // pixels per image block of a step
  int hm[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int tp = xw_pixel(ks, lg, h, lq);
      if constexpr (GEN) {
        const int pr = tp / p.seg;
        hm[ks][h] = pr * W2 + tp - pr * p.seg;
        continue;
      }
      const int ii = tp / spi, rem = tp - ii * spi;
      const int pr = rem / p.W, q = rem - pr * p.W;
      hm[ks][h] = ii * p.hb + pr * W2 + q;
    }
  const int wm = wave >> 1, wn = wave & 1;  // wave row (144 of the 576 GEMM rows) and column half (32 channels)
  // dy fragment (ks, j), tr read h: row xw_pixel(ks, lg, h, lq), 8-B unit wn 8 + 4 j + lp; + 32 rows keeps the
  // swizzle, + 4 units flips bit 2 of the unit: offset (b0[h] ^ 32 j) + 4096 ks
  uint32_t b0[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kr = xw_pixel(0, lg, h, lq);
    b0[h] = (uint32_t)(XW_DY + kr * 128 + (((wn * 8 + lp) ^ f32x_uswz(kr)) << 3));
  }

  f32x4 acc[9][2], lo[9][2];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = lo[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const char* sb, const int (&hr)[2][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 bd[3][2];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          bd[pl][j] = f32x_tr8(sb + pl * XW_DPL + ks * 4096, b0[0] ^ (uint32_t)(j * 32), b0[1] ^ (uint32_t)(j * 32));
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const int row = wm * 144 + i * 16;  // GEMM row = tap 64 + channel
        const int tap = row >> 6, unit = ((row & 63) >> 2) + lp;
        const int toff = halo_tap_shift<1>(tap, W2, 0);
        uint32_t ao[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int ra = hr[ks][h] + toff;
          ao[h] = (uint32_t)(ra * 128 + ((unit ^ f32x_uswz(ra)) << 3));
        }
        bf16x8 ax[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) ax[pl] = f32x_tr8(sb + pl * XW_HPL, ao[0], ao[1]);
        constexpr int PX[6] = {2, 1, 0, 1, 0, 0}, PD[6] = {0, 1, 2, 0, 1, 0};  // (x plane, dy plane)
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (q < 5) lo[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[PX[q]], bd[PD[q]][j], lo[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[0], bd[0][j], acc[i][j], 0, 0, 0);
      }
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
      char* const sb = smem + ((k - st_begin) & 1) * XW_STAGE;
      char* const nb = smem + ((k - st_begin + 1) & 1) * XW_STAGE;
      const bool more = k + 1 < st_end;
      if (more) load_step(k + 1);
      __builtin_amdgcn_sched_barrier(0);
      int hr[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          hr[ks][h] = hm[ks][h];
          asm volatile("" : "+v"(hr[ks][h]));
        }
      compute(sb, hr);
      __builtin_amdgcn_sched_barrier(0);
      if (more) write_step(nb);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }

  // ---- epilogue: out[k][tap C + c0 + c] (4 consecutive c per lane: one 16-B store)
  const int RSC = 9 * p.C;
  float* const out = p.out + (size_t)split * p.K * RSC;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int row = wm * 144 + i * 16 + 4 * lg;
    const int rsc = (row >> 6) * p.C + c0 + (row & 63);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kout = k0 + wn * 32 + j * 16 + li;
      *(f32x4*)(out + (size_t)kout * RSC + rsc) = (acc[i][j] + lo[i][j]) * p.scale;
    }
  }
  stamp_end(p.ts);
}

// ---------------------------------------------------------------- host side
struct XwGeom {
  int rows = 0, imgs = 0, hb = 0, nh = 0, nsteps = 0;
  bool gen = false;  // the general instance: `rows` rows x one g.seg-column segment of one image per step
  SegTile g;
};
// Step geometry of a feasible shape: 64 pixels are whole rows of one image or whole images (a last step of fewer
// images than `imgs` is padded with zeros by the loads)
static bool xw_geometry(const ConvShape& s, XwGeom& g) {
  if (!conv3x3_ok(s, 1)) return false;
  if (s.W != 4 && s.W != 8 && s.W != 16 && s.W != 32) return false;
  TileSplit t;
  if (!classic_tile(s.H, s.W, 64, t)) return false;
  g.rows = t.rows;
  g.imgs = t.imgs;
  g.hb = halo_box_s1(t.rows, s.W);
  g.nh = t.imgs * g.hb;
  // 32-bit byte offsets of the fp32 tensors (the buffer descriptors' range; DMA_OOB must lie outside it)
  if (g.nh > XW_HROWS || (uint64_t)s.N * s.H * s.W * std::max(s.C, s.K) * 4 >= (1ull << 31)) return false;
  g.nsteps = t.imgs == 1 ? s.N * (s.H / t.rows) : (s.N + t.imgs - 1) / t.imgs;
  return true;
}

// General geometry of a feasible shape. The step rule: over the divisors seg <= 64 of W, with rs = the largest row
// count <= 64 / seg that divides H, the pair with the most pixels rs seg, ties to the larger seg (fewer side halo
// columns), among those whose halo (rs + 2) x (seg + 2) fits the 144 rows and whose padded slots' tr reads stay inside
// them at the largest tap shift. (224: 32 x 2, 112: 16 x 4, 56: 8 x 8 -- in LDS the classic 32- / 16- / 8-wide steps --
// 28: 28 x 2 = 56 pixels, 14 and 7: 7 x 7 = 49, 64: 32 x 2.)
static bool xw_geometry_gen(const ConvShape& s, XwGeom& g) {
  if (!conv3x3_ok(s, 1)) return false;
  int best = 0;
  for (int seg = 1; seg <= std::min(s.W, 64); ++seg) {
    if (s.W % seg) continue;
    const int rs = rows_dividing(s.H, 64 / seg), w2 = seg + 2;
    // slot 63, the last a tr read addresses, at tap (2, 2): its halo row must exist (a padded slot's too)
    if (halo_box_s1(rs, seg) > XW_HROWS || (63 / seg + 2) * w2 + 63 % seg + 2 >= XW_HROWS) continue;
    if (rs * seg >= best) {
      best = rs * seg;
      g.g = seg_tile(s.H, s.W, seg, rs);
    }
  }
  if (best == 0) return false;
  g.gen = true;
  g.rows = g.g.rs;
  g.imgs = 1;
  g.hb = g.nh = halo_box_s1(g.g.rs, g.g.seg);
  // one image of either operand within the per-step buffer descriptors (32-bit byte offsets; DMA_OOB must lie outside
  // them), and the step index within FastDiv's 31 bits. The tensors themselves may pass 2 GiB
  const int64_t nsteps = (int64_t)s.N * g.g.tpi;
  if ((int64_t)s.H * s.W * std::max(s.C, s.K) * 4 >= (1ll << 31) || nsteps >= (1ll << 31)) return false;
  g.nsteps = (int)nsteps;
  return true;
}
// Option f32x_gen for the weight gradient: 0 classic geometry only; 1 the general step classes (seg, rs) that measured
// faster than conv_f32's weight gradient; 2 every feasible one (for measuring, and the small test shapes)
static bool xw_gen_admitted(const XwGeom& g) {
  const int lvl = option_get(OPT_F32X_GEN);
  if (lvl >= 2) return true;
  // measured (profiles/f32_split_gen_wgrad_bench.txt): the five step classes of the 224 / 112 / 56 / 28 and
  // 14 / 7 wide rows -- 32 x 2, 16 x 4, 8 x 8 (64 pixels), 28 x 2 (56), 7 x 7 (49) -- ran 2.0-3.3x faster than
  // conv_f32's weight gradient at every batch measured (32 and 128 or 256), the split's whole min..max range below the
  // exact kernel's. Every other class (odd row counts that leave rs short, other widths) was not measured: refused
  const int seg = g.g.seg, rs = g.g.rs;
  return lvl == 1 && ((seg == 32 && rs == 2) || (seg == 16 && rs == 4) || (seg == 8 && rs == 8) ||
                      (seg == 28 && rs == 2) || (seg == 7 && rs == 7));
}
// the classic geometry first, unchanged; otherwise, under option f32x_gen, the general one
static bool xw_geometry_any(const ConvShape& s, XwGeom& g) {
  if (xw_geometry(s, g)) return true;
  return option_get(OPT_F32X_GEN) != 0 && xw_geometry_gen(s, g) && xw_gen_admitted(g);
}

bool conv_f32x_wgrad_ok(const ConvShape& s) {
  XwGeom g;
  return xw_geometry_any(s, g);
}

size_t conv_f32x_wgrad_workspace(const ConvShape& s) {
  XwGeom g;
  if (!xw_geometry_any(s, g)) return 0;
  const size_t one = (size_t)s.K * 9 * s.C * 4;
  const int splits = f32x_wgrad_splits_on_hand((s.C / 64) * (s.K / 64), g.nsteps, one, SIZE_MAX);
  return splits == 1 ? 0 : splits * one;
}

int conv_f32x_wgrad(const ConvShape& s, const float* x, const float* dy, float* dw, float scale, float* slab,
                    size_t slab_bytes, hipStream_t st, u64* ts) {
  XwGeom g;
  DTC_CHECK_ARG(xw_geometry_any(s, g), "conv_f32x_wgrad: unsupported shape");
  DTC_CHECK_ARG(x && dy && dw && aligned(x, 16) && aligned(dy, 16) && aligned(dw, 16) && (!slab || aligned(slab, 16)),
                "conv_f32x_wgrad: null / misaligned argument");
  const int tiles = (s.C / 64) * (s.K / 64);
  const int splits = f32x_wgrad_splits_on_hand(tiles, g.nsteps, (size_t)s.K * 9 * s.C * 4, slab ? slab_bytes : 0);
  XwParams p{};
  p.x = x; p.dy = dy;
  p.out = splits == 1 ? dw : slab;
  p.scale = splits == 1 ? scale : 1.f;
  p.N = s.N; p.H = s.H; p.W = s.W; p.C = s.C; p.K = s.K;
  p.x_bytes = (uint32_t)((uint64_t)s.N * s.H * s.W * s.C * 4);
  p.dy_bytes = (uint32_t)((uint64_t)s.N * s.H * s.W * s.K * 4);
  p.rows = g.rows; p.imgs = g.imgs; p.hb = g.hb; p.nh = g.nh;
  p.spimg = s.H / g.rows;
  p.nsteps = g.nsteps;
  p.steps_per_split = (g.nsteps + splits - 1) / splits;
  p.ts = ts;
  if (g.gen) {  // one image: the descriptors are made per step
    p.x_bytes = (uint32_t)((uint64_t)s.H * s.W * s.C * 4);
    p.dy_bytes = (uint32_t)((uint64_t)s.H * s.W * s.K * 4);
    p.seg = g.g.seg; p.spr = g.g.spr; p.tpi = g.g.tpi;
    p.fd_tpi = make_fastdiv(g.g.tpi);
    p.fd_spr = make_fastdiv(g.g.spr);
  }
  const dim3 grid((unsigned)tiles, (unsigned)splits);
  if (g.gen) DTC_KLAUNCH(conv_f32x_wgrad_kernel<1>, grid, dim3(512), 0, st, p);
  else DTC_KLAUNCH(conv_f32x_wgrad_kernel<0>, grid, dim3(512), 0, st, p);
  DTC_LAUNCH_CHECK();
  if (splits == 1) return 0;
  return f32_wgrad_reduce(slab, splits, s.K, 9 * s.C, 9 * s.C, 9 * s.C, scale, dw, st, ts);
}

}  // namespace dtc
