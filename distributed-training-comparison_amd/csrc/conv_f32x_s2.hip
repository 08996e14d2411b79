// Split-bf16 transition-block convolutions for the fp32 executor, on the bf16 MFMA (v_mfma_f32_16x16x32_bf16) of
// gfx950: conv1 (3x3 / stride 2 / pad 1) of a projection block and the block's 1x1 stride-2 shortcut in ONE launch,
// forward and data gradient. fp32 NHWC activations in and out, fp32-grade results, conv_f32x.hip's scheme: every fp32
// operand is three bf16 planes (f32_split.h: split8; the weights' planes are f32_split3's), a product is the six
// plane products of order <= 2, accumulated in fp32 in a fixed order. No atomics on outputs, no split-K: bit-identical
// run to run.
//
//   FWD_SC    y   = conv3x3_s2(x, W1)  and  ysc = conv1x1_s2(x, Wsc): the shortcut is the centre tap (1, 1) of the
//             same staged halo against a tenth weight stage, into accumulators of its own -- x is read once.
//   DGRAD_SC  dx  = dgrad_s2(dy, W1) + dgrad_1x1_s2(dsc, Wsc) in sub-pixel (parity-class) form: dx(2i + a, 2j + b)
//             takes the taps with r - 1 = a, s - 1 = b (mod 2) -- 1 / 2 / 2 / 4 taps for classes (0,0) (0,1) (1,0)
//             (1,1) -- from the dy box at offsets (da, db) in {0, 1}^2; the shortcut is a tenth tap of class (0,0)
//             from dsc. Every dx pixel is written exactly once (the extents are even): no residual pass.
//
//   pass      D = A x B (MFMA rows x cols)   A (rows, from LDS)                       B (cols)
//   FWD_SC    y / ysc[k][position]           W planes [k][tap][c-chunk]   row image   column-split halo of x, + tap shift
//   DGRAD_SC  dx[c][class][position]         W planes [k-chunk][tap][c]   tr image    dy box at + (da, db) / dsc rows
//
// Tile: 64 output channels x 32 positions of the [N][H/2][W/2] grid (whole rows of one image, or whole images) per
// 256-thread workgroup; wave (wk, wp) owns channels 32 wk .. + 31 of positions 16 wp .. + 15: 2 x 1 fragments, 24
// MFMAs per step (FWD) -- the 64-position tile of the stride-1 kernel does not fit: its input box is 306 .. 360 halo
// rows, 138 KB of three 128-B-row planes. 32 positions need 170 (2 rows of 16), 162 (4 rows of 8) and 180 (two 4x4
// images) halo rows at pitch 2 (wo + 1), the reduction chunk stays 64 channels (128-B rows), and every
// tile_common.h layout rule (hswz, halo_frag_off, frag_row, frag_tr) is used as it is.
// Activations: per 64-channel chunk each thread loads its (halo row, 8-channel) units -- 6 (FWD) / 3 (DGRAD: two of
// the dy box, one of the dsc rows) -- with two bounds-checked 16-B buffer loads each (out-of-image pixels: DMA_OOB,
// zeros, no branch), one unit per step of the PREVIOUS chunk; at the chunk boundary it splits them (once per halo
// element, not once per tap) and writes the three plane images. FWD: the column-split stride-2 halo (halo_box_col<2>,
// halo_tap_shift<2>): every tap is a constant shift of halo rows. DGRAD: the stride-1 (rows + 1) x (wo + 1) box.
// Weights: a step's 3 x 8 KB planes go global -> LDS by LDS-DMA into one of two buffers during the previous step's
// MFMAs; ten steps per chunk (nine taps + the shortcut), so a step's buffer is its parity.
// Accumulators, per fragment: acc -- the (0,0) products of ONE chunk (<= 18 MFMAs), added into tot by VALU at the
// chunk boundary; lo1 -- the order-1 corrections (0,1) (1,0); lo2 -- the order-2 ones (0,2) (1,1) (2,0). The
// per-chunk set is kept on measurement: with the fold compiled out the worst error over the test shapes grows with
// the reduction (7.1e-8 of sum |x||w| at 9 x 64, 1.03e-7 at 9 x 256 forward, 1.10e-7 at K = 512 data gradient; the
// bound is 2.4e-7) where with it it stays flat (2.9e-8 at 9 x 256), the predicate does not bound C or K, and the set
// costs 8 (FWD) / 32 (DGRAD) registers in kernels that are not register-bound. The two correction sets (instead of
// one) give four independent MFMA chains per wave. The shortcut's sets are folded the same way. DGRAD holds the four
// classes' sets at once: 4 x 4 x 2 fragments = 128 registers, which is why a workgroup takes 32 positions and a wave
// one position fragment.
//
// LDS map, FWD_SC (122,880 B; one workgroup per CU):     DGRAD_SC (86,016 B; one workgroup per CU):
//   [0, 73728)        three halo images of 192 rows        [0, 36864)       three images of 96 rows: 64 of the dy
//   [73728, 122880)   two weight buffers of 3 x 8 KB                        box, then the 32 positions' dsc rows
//   (epilogue: [0, 2048) BN statistics staging, y / ysc)   [36864, 86016)   two weight buffers of 3 x 8 KB
// Registers: 256 (FWD_SC: 200 VGPR + 56 AGPR) / 300 (DGRAD_SC: 192 + 108) of 512; no scratch.
#include "common.h"
#include "f32_split.h"
#include "flat.h"
#include "kernels.h"
#include "tile_common.h"

namespace dtc {

enum { S2X_FWD = 0, S2X_DGRAD = 1 };

constexpr int S2X_BM = 64, S2X_BN = 32, S2X_NST = 10;
constexpr int S2X_WBYTES = S2X_BM * 128;  // one weight plane of one step
constexpr int S2X_WTAP = 3 * S2X_WBYTES;  // one step's three planes
constexpr int S2X_FCAP = 192;             // FWD halo rows
constexpr int S2X_DBOX = 64, S2X_DCAP = S2X_DBOX + S2X_BN;  // DGRAD: dy box rows, then the dsc rows

struct S2xParams {
  const float* src;   // FWD x [N][H][W][C]; DGRAD dy [N][Ho][Wo][K]
  const float* src2;  // DGRAD dsc [N][Ho][Wo][K]
  const u16* w;       // three bf16 planes of W1 [K][3][3][C], wstride elements apart
  const u16* wsc;     // three bf16 planes of Wsc [K][C], wsc_stride elements apart
  int64_t wstride, wsc_stride;
  float* out;         // FWD y [N][Ho][Wo][K]; DGRAD dx [N][H][W][C]
  float* out2;        // FWD ysc
  int64_t* stats;     // FWD: BN statistics slots of y / ysc, or null
  int64_t* stats2;
  int N, H, W, C, K, Ho, Wo;
  uint32_t src_bytes;
  int rows, imgs, hb, nh, tiles_y, tiles_a, nchunk, xcd_remap;
  u64* ts;
};

// Position of B-fragment column j within its 16 positions: for 8- and 4-wide rows columns {4..11} and {0..3, 12..15}
// each take two row pieces whose halo rows are distinct mod 8 (FWD: output rows are 2 pitches = 36 / 20 halo rows
// apart; DGRAD: 9 / 5), as halo_frag_off's conflict-free ds_read_b128 wants
__device__ __forceinline__ int s2x_frag_pos(int j, int wo) {
  return wo == 16 ? j : (j >= 4 && j < 12) ? j - 4 : (j < 4 ? j + 8 : j);
}

template <int PASS>
__global__ void __launch_bounds__(256) conv_f32x_s2_kernel(const S2xParams p) {
  constexpr bool FWD = PASS == S2X_FWD;
  constexpr int HCAP = FWD ? S2X_FCAP : S2X_DCAP;
  constexpr int HBYTES = HCAP * 128;     // one halo image
  constexpr int UNITS = HCAP * 8 / 256;  // (halo row, 8-channel) units per thread and chunk: 6 / 3
  constexpr int FM = 2;                  // channel fragments per wave (one position fragment)
  constexpr int NCL = FWD ? 2 : 4;       // accumulator families: FWD y, ysc; DGRAD the four parity classes
  constexpr int NB = FWD ? 9 : 5;        // B offsets: FWD the nine taps; DGRAD the four box offsets + the dsc rows
  // DGRAD step t < 9: box offset 2 da + db, class 2 py + px, weight tap 3 r + s (each tap once; offset-major, so an
  // offset's B fragments are read once for all its classes)
  constexpr int DT_OFF[9] = {0, 0, 0, 0, 1, 1, 2, 2, 3};
  constexpr int DT_CLS[9] = {0, 1, 2, 3, 1, 3, 2, 3, 3};
  constexpr int DT_TAP[9] = {4, 5, 7, 8, 3, 6, 1, 2, 0};
  __shared__ __attribute__((aligned(1024))) char smem[3 * HBYTES + 2 * S2X_WTAP];
  char* const wbase = smem + 3 * HBYTES;

  stamp_start(p.ts);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wk = wave >> 1, wp = wave & 1;
  int bid = blockIdx.x;
  if (p.xcd_remap && gridDim.x >= 16) bid = (int)xcd_grouped_id(blockIdx.x, gridDim.x);
  const int ta = bid % p.tiles_a, tb = bid / p.tiles_a;
  const int a0 = ta * S2X_BM;  // first output channel: FWD k, DGRAD c
  int n0, y0;                  // first image and first row of the [Ho][Wo] grid
  if (p.imgs == 1) {
    n0 = tb / p.tiles_y;
    y0 = (tb - n0 * p.tiles_y) * p.rows;
  } else {
    n0 = tb * p.imgs;
    y0 = 0;
  }
  const int pos0 = (n0 * p.Ho + y0) * p.Wo;  // the tile's 32 slots are positions pos0 .. pos0 + 31
  const int npos = p.N * p.Ho * p.Wo;
  const int lrow = lane >> 3, pc = lane & 7;
  const int RSC = 9 * p.C;
  const int hwh = p.Wo + 1, pitch = 2 * hwh;  // FWD: even box columns per halo row pitch; DGRAD: hwh is the box width

  // ---- weight DMA: per-lane element offsets within a plane (add the step's tap / chunk term)
  int offW[2], offS[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (wave + 4 * j) * 8 + lrow;
    if constexpr (FWD) {  // row image: LDS row = output channel k, 64 input channels of one tap
      offW[j] = (a0 + row) * RSC + (pc ^ rowswz(row)) * 8;
      offS[j] = (a0 + row) * p.C + (pc ^ rowswz(row)) * 8;
    } else {  // tr image: LDS row = k within the chunk, the tile's 64 channels c
      offW[j] = row * RSC + a0 + (pc ^ trswz(row)) * 8;
      offS[j] = row * p.C + a0 + (pc ^ trswz(row)) * 8;
    }
  }
  auto stage_w = [&](char* dst, int cc, int st) {  // step st of chunk cc: a tap of W1, or (9) the shortcut's Wsc
    const u16* src;
    int64_t stride;
    if (st == 9) {
      src = p.wsc + (FWD ? cc * 64 : cc * 64 * p.C);
      stride = p.wsc_stride;
    } else {
      src = p.w + (FWD ? st * p.C + cc * 64 : cc * 64 * RSC + DT_TAP[st] * p.C);
      stride = p.wstride;
    }
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        glds16(src + pl * stride + (st == 9 ? offS[j] : offW[j]), dst + pl * S2X_WBYTES + (wave + 4 * j) * 1024);
  };

  // ---- halo units: unit u of this thread is halo row (u 256 + t) / 8, channels 8 (t % 8) .. + 7
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs2 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(FWD ? p.src : p.src2), 0, p.src_bytes, 0x00020000);
  uint32_t hoff[UNITS];  // byte offset of the unit in chunk 0 (DMA_OOB: a padded pixel / an empty slot, loads zeros)
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    const int hr = (u * 256 + t) >> 3;
    uint32_t off = DMA_OOB;
    if constexpr (FWD) {
      if (hr < p.nh) {
        const int i = hr / p.hb, rem = hr - i * p.hb;
        const int by = rem / pitch, hx = rem - by * pitch;
        const int col = halo_box_col<2>(hx, hwh);
        const int n = n0 + i, y = 2 * y0 - 1 + by, x = col - 1;
        if (col >= 0 && n < p.N && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
          off = (uint32_t)((((n * p.H + y) * p.W + x) * p.C + pc * 8) * 4);
      }
    } else if (hr >= S2X_DBOX) {  // (unit 2) the dsc row of slot hr - 64
      const int pos = pos0 + hr - S2X_DBOX;
      if (pos < npos) off = (uint32_t)((pos * p.K + pc * 8) * 4);
    } else if (hr < p.nh) {  // the dy box: bottom / right neighbours beyond the image are zeros
      const int i = hr / p.hb, rem = hr - i * p.hb;
      const int ry = rem / hwh, rx = rem - ry * hwh;
      const int n = n0 + i, a = y0 + ry;
      if (n < p.N && a < p.Ho && rx < p.Wo) off = (uint32_t)((((n * p.Ho + a) * p.Wo + rx) * p.K + pc * 8) * 4);
    }
    hoff[u] = off;
  }
  f32x4 pf[UNITS][2];  // the next chunk's halo, fp32, in flight / held until the chunk boundary
  auto load_unit = [&](int u, int cc) {
    const uint32_t o = hoff[u] == DMA_OOB ? DMA_OOB : hoff[u] + (uint32_t)(cc * 256);
    const __amdgpu_buffer_rsrc_t r = (!FWD && u == UNITS - 1) ? rs2 : rs;
    f32x_load16(r, o, pf[u]);
  };
  auto write_halo = [&]() {  // split the held chunk and write its three images
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
      const int hr = (u * 256 + t) >> 3;
      const float v[8] = {pf[u][0][0], pf[u][0][1], pf[u][0][2], pf[u][0][3],
                          pf[u][1][0], pf[u][1][1], pf[u][1][2], pf[u][1][3]};
      uint4 q0, q1, q2;
      split8(v, q0, q1, q2);
      char* const dst = smem + hr * 128 + ((pc ^ hswz(hr)) << 4);
      *(uint4*)dst = q0;
      *(uint4*)(dst + HBYTES) = q1;
      *(uint4*)(dst + 2 * HBYTES) = q2;
    }
  };

  // ---- B fragments: this lane's position (slot), its halo row at tap / offset (0, 0), then every B offset
  const int slot = wp * 16 + s2x_frag_pos(lane & 15, p.Wo);
  uint32_t boff[NB];
  {
    const int spx = p.rows * p.Wo;  // positions per image slice
    const int i = slot / spx, rem = slot - i * spx;
    const int y = rem / p.Wo, x = rem - y * p.Wo;
    if constexpr (FWD) {
      const int hbr = i * p.hb + 2 * y * pitch + x;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) boff[tap] = halo_frag_off(hbr + halo_tap_shift<2>(tap, pitch, hwh), lane);
    } else {
      const int hbr = i * p.hb + y * hwh + x;
#pragma unroll
      for (int o = 0; o < 4; ++o) boff[o] = halo_frag_off(hbr + (o >> 1) * hwh + (o & 1), lane);
      boff[4] = halo_frag_off(S2X_DBOX + slot, lane);
    }
  }

  f32x4 acc[NCL][FM], tot[NCL][FM], lo1[NCL][FM], lo2[NCL][FM];
#pragma unroll
  for (int c = 0; c < NCL; ++c)
#pragma unroll
    for (int i = 0; i < FM; ++i) acc[c][i] = tot[c][i] = lo1[c][i] = lo2[c][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  typedef __attribute__((address_space(3))) bf16x8 lds_bf16x8;
  // one 32-deep k-step of family c: the six plane products, (weight plane, activation plane) = (2,0) (1,0) (1,1)
  // (0,1) (0,2) (0,0); consecutive MFMAs never share an accumulator, the same accumulator comes back every fourth
  auto mma6 = [&](const bf16x8 (&aw)[3][FM], const bf16x8 (&bx)[3], int c) {
    constexpr int PW[6] = {2, 1, 1, 0, 0, 0}, PX[6] = {0, 0, 1, 1, 2, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if (q == 5) acc[c][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[0][i], bx[0], acc[c][i], 0, 0, 0);
        else if (q & 1) lo1[c][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[PW[q]][i], bx[PX[q]], lo1[c][i], 0, 0, 0);
        else lo2[c][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[PW[q]][i], bx[PX[q]], lo2[c][i], 0, 0, 0);
      }
  };
  bf16x8 bkeep[2][3];  // DGRAD: an offset's B fragments, kept over the steps (classes) that use it
  auto compute = [&](const char* wb, int st) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 aw[3][FM];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          if constexpr (FWD) aw[pl][i] = frag_row(wb + pl * S2X_WBYTES, wk * 32 + i * 16, ks, lane);
          else aw[pl][i] = frag_tr(wb + pl * S2X_WBYTES, wk * 32 + i * 16, ks, lane);
        }
      if constexpr (FWD) {  // the shortcut (step 9) reads the centre tap
        bf16x8 bx[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          bx[pl] = *(const lds_bf16x8*)(smem + pl * HBYTES + (boff[st == 9 ? 4 : st] ^ (uint32_t)(ks * 64)));
        mma6(aw, bx, st == 9 ? 1 : 0);
      } else {
        const int o = st == 9 ? 4 : DT_OFF[st];
        if (st == 0 || st == 4 || st == 6 || st == 8 || st == 9) {
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            bkeep[ks][pl] = *(const lds_bf16x8*)(smem + pl * HBYTES + (boff[o] ^ (uint32_t)(ks * 64)));
        }
        mma6(aw, bkeep[ks], st == 9 ? 0 : DT_CLS[st]);
      }
    }
  };

  // ---- main loop: chunks x 10 unrolled steps. Step s reads weight buffer s & 1; after the step's barrier (every
  // wave is done with the previous step) the next step's weights go to the other buffer and unit s of the next
  // chunk's halo is loaded into registers: both have this step's MFMAs to land, and the next step's s_waitcnt
  // vmcnt(0) finds them done. At a chunk boundary every wave passes a barrier (the halo images are free), splits its
  // held units and writes them; the next step's barrier publishes them.
#pragma unroll
  for (int u = 0; u < UNITS; ++u) load_unit(u, 0);
  stage_w(wbase, 0, 0);
  write_halo();
  for (int c = 0; c < p.nchunk; ++c) {
    const bool more = c + 1 < p.nchunk;
#pragma unroll
    for (int st = 0; st < S2X_NST; ++st) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      char* const wnext = wbase + ((st + 1) & 1) * S2X_WTAP;
      if (st + 1 < S2X_NST) stage_w(wnext, c, st + 1);
      else if (more) stage_w(wnext, c + 1, 0);
      if (st < UNITS && more) load_unit(st, c + 1);
      compute(wbase + (st & 1) * S2X_WTAP, st);
    }
#pragma unroll
    for (int k = 0; k < NCL; ++k)
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        tot[k][i] += acc[k][i];
        acc[k][i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    if (more) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      write_halo();
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // LDS reads done before the epilogue reuses smem
  asm volatile("" ::: "memory");

  // ---- epilogue: D[row = channel a0 + 32 wk + 16 i + 4 (lane >> 4) + v][col = this lane's position]
  const int rq = (lane >> 4) * 4;
  const int pos = pos0 + slot;
  const bool ok = pos < npos;  // (false: a padded image slot of the last tile)
  const int ch0 = a0 + wk * 32 + rq;
  if constexpr (FWD) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // y, then ysc
      float* const out = k == 0 ? p.out : p.out2;
      int64_t* const stats = k == 0 ? p.stats : p.stats2;
      float* const red = (float*)smem + k * (2 * S2X_BM * 2);  // [2 position halves][S2X_BM][2]
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const f32x4 d = tot[k][i] + (lo1[k][i] + lo2[k][i]);
        if (ok) *(f32x4*)(out + (size_t)pos * p.K + ch0 + i * 16) = d;
        if (stats != nullptr) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const float dv = ok ? d[v] : 0.f;
            const float s = row16_sum(dv), q = row16_sum(dv * dv);
            if ((lane & 15) == 0) {
              red[(wp * S2X_BM + wk * 32 + i * 16 + rq + v) * 2 + 0] = s;
              red[(wp * S2X_BM + wk * 32 + i * 16 + rq + v) * 2 + 1] = q;
            }
          }
        }
      }
      if (stats != nullptr) stats_fold<2, S2X_BM>(red, stats, p.K, a0);
    }
  } else if (ok) {  // class (py, px) of position (n, a, b) -> dx pixel (n, 2 a + py, 2 b + px)
    const int hw = p.Ho * p.Wo;
    const int n = pos / hw, rem = pos - n * hw;
    const int a = rem / p.Wo, b = rem - a * p.Wo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t o = ((size_t)(n * p.H + 2 * a + (k >> 1)) * p.W + 2 * b + (k & 1)) * p.C + ch0;
#pragma unroll
      for (int i = 0; i < FM; ++i) *(f32x4*)(p.out + o + i * 16) = tot[k][i] + (lo1[k][i] + lo2[k][i]);
    }
  }
  stamp_end(p.ts);
}

// ---------------------------------------------------------------- host side
// Tile geometry of a feasible shape: 32 positions of the output grid are whole rows of one image or whole images
static bool s2x_geometry(const ConvShape& s, TileSplit& t) {
  if (!conv3x3_ok(s, 2) || s.H % 2 || s.W % 2) return false;
  const int ho = s.H / 2, wo = s.W / 2;
  if (wo != 4 && wo != 8 && wo != 16) return false;  // the rows s2x_frag_pos covers
  if (!classic_tile(ho, wo, S2X_BN, t)) return false;
  // FWD: the column-split box at pitch 2 (wo + 1) (s2_pitch's padding only serves tr reads); DGRAD: the dy box
  const int nhf = t.imgs * (2 * t.rows + 1) * 2 * (wo + 1), nhd = t.imgs * halo_box_subpixel(t.rows, wo);
  // 32-bit byte offsets of the fp32 tensors (the buffer descriptor's range; DMA_OOB must lie outside it)
  // and 32-bit element offsets into a weight plane
  return nhf <= S2X_FCAP && nhd <= S2X_DBOX && (uint64_t)s.N * s.H * s.W * s.C * 4 < (1ull << 31) &&
         (uint64_t)s.N * ho * wo * s.K * 4 < (1ull << 31) && (uint64_t)s.K * 9 * s.C < (1ull << 31);
}

// DGRAD_SC: every feasible geometry (measured 4.4-7.0x over the exact pair). FWD_SC: where it measured
// faster than the two conv_f32 launches by more than either column's spread, at batches 32 / 64 / 128 / 256 of the
// model's three shapes: layer 2 wins to batch 64 (1.06x; 0.92x at 128), layer 3 at all four (1.06x at 256), layer 4
// to batch 128 (1.52x; 1.00x at 256). Larger problems than the largest measured win are refused
bool conv_f32x_s2_ok(const ConvShape& s, int pass) {
  TileSplit t;
  if (!s2x_geometry(s, t)) return false;
  if (pass != CONV_FWD) return pass == CONV_DGRAD;
  if (option_get(OPT_F32X_S2_FWD) >= 2) return true;  // every feasible geometry: for measuring the refused ones
  // work in (tile, output-channel tile, chunk) units, up to the largest measured size at which this row width won:
  // 16-wide rows (layer 2) batch 64, 8-wide (layer 3) batch 256, the largest measured, 4-wide (layer 4) batch 128.
  // Other channel counts of the same row width are taken at equal units: extrapolated, not measured
  const int wo = s.W / 2;
  const int64_t tiles = t.imgs == 1 ? (int64_t)s.N * (s.H / 2 / t.rows) : (s.N + t.imgs - 1) / t.imgs;
  return tiles * (s.K / S2X_BM) * (s.C / 64) <= (wo == 16 ? 1024 : wo == 8 ? 4096 : 2048);
}

static int s2x_launch(const ConvShape& s, int pass, S2xParams& p, hipStream_t st, u64* ts) {
  TileSplit t;
  DTC_CHECK_ARG(s2x_geometry(s, t), "conv_f32x_s2: unsupported shape");
  DTC_CHECK_ARG(p.src && p.w && p.wsc && p.out && (pass == S2X_FWD ? p.out2 != nullptr : p.src2 != nullptr) &&
                    p.wstride >= (int64_t)s.K * 9 * s.C && p.wsc_stride >= (int64_t)s.K * s.C && p.wstride % 8 == 0 &&
                    p.wsc_stride % 8 == 0 && aligned(p.w, 16) && aligned(p.wsc, 16) && aligned(p.src, 16) &&
                    aligned(p.out, 16) && (!p.src2 || aligned(p.src2, 16)) && (!p.out2 || aligned(p.out2, 16)),
                "conv_f32x_s2: null / misaligned argument or weight planes closer than one filter bank");
  p.N = s.N; p.H = s.H; p.W = s.W; p.C = s.C; p.K = s.K;
  p.Ho = s.H / 2; p.Wo = s.W / 2;
  p.rows = t.rows; p.imgs = t.imgs;
  p.hb = pass == S2X_FWD ? (2 * t.rows + 1) * 2 * (p.Wo + 1) : halo_box_subpixel(t.rows, p.Wo);
  p.nh = t.imgs * p.hb;
  p.src_bytes = pass == S2X_FWD ? (uint32_t)((uint64_t)s.N * s.H * s.W * s.C * 4)
                                : (uint32_t)((uint64_t)s.N * p.Ho * p.Wo * s.K * 4);
  p.tiles_y = p.Ho / t.rows;
  p.tiles_a = (pass == S2X_FWD ? s.K : s.C) / S2X_BM;
  p.nchunk = (pass == S2X_FWD ? s.C : s.K) / 64;
  p.xcd_remap = option_get(OPT_XCD_REMAP);
  p.ts = ts;
  const int tiles_b = t.imgs == 1 ? s.N * p.tiles_y : (s.N + t.imgs - 1) / t.imgs;
  const dim3 grid((unsigned)(tiles_b * p.tiles_a), 1);
  if (pass == S2X_FWD) DTC_KLAUNCH(conv_f32x_s2_kernel<S2X_FWD>, grid, dim3(256), 0, st, p);
  else DTC_KLAUNCH(conv_f32x_s2_kernel<S2X_DGRAD>, grid, dim3(256), 0, st, p);
  DTC_LAUNCH_CHECK();
  return 0;
}

int conv_f32x_s2_fwd(const ConvShape& s, const float* x, const u16* wplanes, int64_t wstride, float* y, int64_t* stats,
                     const u16* wsc_planes, int64_t wsc_stride, float* ysc, int64_t* stats_sc, hipStream_t st, u64* ts) {
  S2xParams p{};
  p.src = x; p.w = wplanes; p.wstride = wstride; p.wsc = wsc_planes; p.wsc_stride = wsc_stride;
  p.out = y; p.out2 = ysc; p.stats = stats; p.stats2 = stats_sc;
  return s2x_launch(s, S2X_FWD, p, st, ts);
}

int conv_f32x_s2_dgrad(const ConvShape& s, const float* dy, const u16* wplanes, int64_t wstride, float* dx,
                       const float* dsc, const u16* wsc_planes, int64_t wsc_stride, hipStream_t st, u64* ts) {
  S2xParams p{};
  p.src = dy; p.src2 = dsc; p.w = wplanes; p.wstride = wstride; p.wsc = wsc_planes; p.wsc_stride = wsc_stride;
  p.out = dx;
  return s2x_launch(s, S2X_DGRAD, p, st, ts);
}

}  // namespace dtc
