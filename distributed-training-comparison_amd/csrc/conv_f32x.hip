// Split-bf16 3x3 / stride 1 / pad 1 convolution for the fp32 executor, forward and data-gradient, on the bf16
// MFMA (v_mfma_f32_16x16x32_bf16) of gfx950: fp32 NHWC activations in and out, fp32-grade results.
//
// gfx950 has no xf32; conv_f32.hip's v_mfma_f32_16x16x4_f32 runs at the fp32 vector rate. Here every fp32 operand
// a is split into three bf16 planes a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1) (round to nearest
// even; both subtractions are exact in fp32, and a0 + a1 + a2 == a), and the product a * w is the six plane
// products of order i + j <= 2: (0,0) (0,1) (1,0) (0,2) (1,1) (2,0), accumulated in fp32 in a fixed order: the (0,0)
// products per 64-channel chunk and the chunks by VALU adds, the five corrections in a set of their own (added in
// the epilogue). The dropped terms are below 2^-24 of |a||w|. No atomics on outputs, no split-K: bit-identical
// run to run.
//
//   pass    D = A x B (MFMA rows x cols)   A (rows, from LDS)                      B (cols)
//   FWD     y[k][pixel]                     W planes [k][r][s][c-chunk]  row image  halo planes of x  at +(r, s)
//   DGRAD   dx[c][pixel]                    W planes [k-chunk][r][s][c]  tr image   halo planes of dy at +(2-r, 2-s)
//
// Tile: 64 output channels x 128 pixels (whole image rows, or whole images of 8x8 / 4x4) per 256-thread workgroup;
// wave w owns all 64 channels of pixels 32 w .. 32 w + 31: 4 x 2 fragments of 16x16, 48 MFMAs per 32-deep k-step.
// Activations: they are fp32 in HBM, so they cannot be LDS-DMA'd as bf16. Per 64-channel reduction chunk each thread
// loads nine (halo row, 8-channel) units of the zero-padded (rows + 2) x (W + 2) halo with two 16-B buffer loads
// each (out-of-image pixels: an offset outside the descriptor, which loads zeros -- no branch), one unit per tap
// step of the PREVIOUS chunk; at the chunk boundary it splits them with plain VALU (cast, subtract, cast, subtract,
// cast: once per halo element, not once per tap) and writes three bf16 halo images in conv_halo's layout (128-B rows,
// tile_common.h's hswz swizzle). All nine taps read ds_read_b128 fragments of each image shifted by r (W + 2) + s.
// Weights: three bf16 KRSC planes made once per forward by f32_split3 (below); a tap's 3 x 8 KB are staged
// global -> LDS by LDS-DMA (asm form, counted by s_waitcnt vmcnt) into one of two buffers, the next tap's during
// the current tap's MFMAs. DGRAD reads W transposed with ds_read_b64_tr_b16 (frag_tr): nothing is transposed in HBM.
// Epilogues: FWD stores fp32 y and, with `stats`, adds the per-channel sum and sum of squares into the int64
// fixed-point BN slots exactly as conv_f32_kernel<F32_FWD> does (stats_fold / stat_add, slot blockIdx.x mod 8);
// DGRAD stores fp32 dx (+ an fp32 residual).
//
// LDS map (159,744 B of 163,840; one workgroup per CU):
//   [0, 110592)        three halo images (plane 0, 1, 2) of 288 rows x 128 B
//   [110592, 159744)   two weight buffers of three planes x 64 rows x 128 B
//   (epilogue: [0, 2048) the BN statistics staging [4 waves][64 channels][2])
// Registers: 357 (FWD) / 360 (DGRAD) of 512 (256 VGPR + 101 / 104 AGPR); no scratch. The general-geometry instances
// (GEN = 1, at the kernel): the same LDS map, 361 / 364 registers, no scratch.
#include "common.h"
#include "f32_split.h"
#include "flat.h"
#include "kernels.h"
#include "tile_common.h"

namespace dtc {

enum { FX_FWD = 0, FX_DGRAD = 1 };

constexpr int FX_BM = 64, FX_BN = 128, FX_HCAP = 288;
constexpr int FX_HBYTES = FX_HCAP * 128;       // one halo image
constexpr int FX_WBYTES = FX_BM * 128;         // one weight plane of one tap
constexpr int FX_WTAP = 3 * FX_WBYTES;         // one tap's three planes
constexpr int FX_UNITS = FX_HCAP * 8 / 256;    // (halo row, 8-channel) units per thread and chunk
static_assert(FX_UNITS == 9, "one halo unit per tap step");

struct FxParams {
  const float* src;  // FWD x, DGRAD dy: NHWC fp32, Cin channels
  const u16* w;      // three bf16 KRSC planes [3][wstride], plane p of w[k][r][s][c] at p * wstride + ((k 3 + r) 3 + s) C + c
  int64_t wstride;
  float* out;        // NHWC fp32, Cout channels
  const float* res;  // DGRAD residual or null
  int64_t* stats;    // FWD BN statistics slots or null
  int N, H, W, Cin, Cout, C;
  uint32_t src_bytes;
  int rows, imgs, hb, nh, tiles_y, tiles_a, nchunk, xcd_remap;
  u64* ts;
  // general geometry (GEN): a tile is rs rows x one seg-column segment of one image, each tile row padded to segp slots
  int seg, segp, rs, spr, tpi;
  FastDiv fd_tpi, fd_spr, fd_segp, fd_w2;
};

// ---------------------------------------------------------------- the split
// The public split (dtc_f32_split3; the weight planes of the executor): as above, with the two edges closed so that
// (p2 + p1) + p0 == a bit for bit for every finite a whose last bit is at or above 2^-133 (the bf16 subnormal step):
// a finite a that would round up to bf16 infinity is truncated instead (its remainder is still exact), and a zero
// remainder takes a's sign (so -0 comes back as -0). NaN gives three NaNs; an infinity gives (inf, NaN, NaN).
struct Split3 {
  const float* src;
  u16* planes;
  int64_t stride;
  __device__ void operator()(int64_t i) const {
    const float a = src[i];
    const uint32_t ab = __float_as_uint(a);
    u16 h0 = f2bf(a);
    if ((h0 & 0x7fffu) == 0x7f80u && (ab & 0x7fffffffu) < 0x7f800000u) h0 = (u16)(ab >> 16);
    const float r1 = a - bf2f(h0);
    u16 h1 = f2bf(r1);
    const float r2 = r1 - bf2f(h1);
    u16 h2 = f2bf(r2);
    const u16 sg = h0 & 0x8000u;
    if ((h1 & 0x7fffu) == 0) h1 = sg;
    if ((h2 & 0x7fffu) == 0) h2 = sg;
    planes[i] = h0;
    planes[stride + i] = h1;
    planes[2 * stride + i] = h2;
  }
};

int f32_split3(const float* src, u16* planes, int64_t n, int64_t stride, hipStream_t st) {
  DTC_CHECK_ARG(src && planes && n > 0 && stride >= n, "f32_split3: bad args");
  return launch_map(n, 2048, st, Split3{src, planes, stride});
}

// Pixel of B-fragment column j within its 16-pixel block (the halo family's permutation for 8- and 4-wide rows:
// columns {4..11} and {0..3, 12..15} must each map to halo rows distinct mod 8 for conflict-free ds_read_b128)
__device__ __forceinline__ int fx_frag_pixel(int j, int W) {
  if (W == 8) return (j >= 4 && j < 12) ? j - 4 : (j < 4 ? j + 8 : j);
  if (W == 4) return (j >= 4 && j < 8) ? j - 4 : (j < 4 ? j + 4 : j);
  return j;
}

// GEN = 1, the general (row segment) geometry of tile_common.h, for rows the classic tile does not cover (224 / 112 /
// 56 / 28 / 14 / 7 wide): a tile is rs rows x one seg-column segment (seg = row_segment(W)) of ONE image, its halo the
// (rs + 2) x (seg + 2) box around it, whose border is padding only where it leaves the image (beside another segment
// or tile it holds that neighbour's pixels). Slots: every tile row is padded to segp = seg rounded up to 16 slots, slot
// l = row l / segp, column l % segp, valid iff the column is below seg and the row below rs. A 16-pixel B fragment is
// then 16 consecutive pixels of one tile row = 16 consecutive halo rows, the conflict-free case of the classic 16- /
// 32-wide rows (a dense l / seg mapping would let a fragment straddle two rows of a 56- or 28-wide segment, whose halo
// rows collide mod 8). A padded slot reads halo rows of its own (in capacity; every row of the images is written each
// chunk), and an MFMA column only feeds its own output column: its result is never stored nor counted.
// Addressing: the buffer descriptor covers the tile's image only (base src + n0 H W Cin), so the 32-bit offsets hold
// for tensors past 2 GiB; output, residual and statistics offsets are 64-bit.
template <int PASS, int GEN>
__global__ void __launch_bounds__(256) conv_f32x_kernel(const FxParams p) {
  constexpr int FM = FX_BM / 16;        // 4 channel fragments per wave
  constexpr int FN = FX_BN / (4 * 16);  // 2 pixel fragments per wave
  constexpr int NIW = FX_BM / 32;       // weight DMA instructions per wave, plane and tap
  __shared__ __attribute__((aligned(1024))) char smem[3 * FX_HBYTES + 2 * FX_WTAP];
  char* const wbase = smem + 3 * FX_HBYTES;

  stamp_start(p.ts);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int bid = blockIdx.x;
  if (p.xcd_remap && gridDim.x >= 16) bid = (int)xcd_grouped_id(blockIdx.x, gridDim.x);
  const int ta = bid % p.tiles_a, tb = bid / p.tiles_a;
  const int a0 = ta * FX_BM;
  int n0, y0, q0 = 0;
  if constexpr (GEN) {
    seg_tile_origin(tb, p.tpi, p.fd_tpi, p.spr, p.fd_spr, p.rs, p.seg, n0, y0, q0);
    n0 = __builtin_amdgcn_readfirstlane(n0);  // (the descriptor below is per tile: keep its base in SGPRs)
  } else if (p.imgs == 1) {
    n0 = tb / p.tiles_y;
    y0 = (tb - n0 * p.tiles_y) * p.rows;
  } else {
    n0 = tb * p.imgs;
    y0 = 0;
  }
  const int W2 = (GEN ? p.seg : p.W) + 2;
  const int px0 = (n0 * p.H + y0) * p.W;
  const int M = p.N * p.H * p.W;
  const int lrow = lane >> 3, pc = lane & 7;
  const int RSC = 9 * p.C;

  // ---- weight DMA: per-lane element offsets within a plane (add the step's tap / chunk term)
  int offW[NIW];
#pragma unroll
  for (int j = 0; j < NIW; ++j) {
    if constexpr (PASS == FX_FWD) {  // row image: LDS row = output channel, 64 input channels of one tap
      const int row = (wave + 4 * j) * 8 + lrow;
      offW[j] = (a0 + row) * RSC + (pc ^ rowswz(row)) * 8;
    } else {  // tr image: LDS row = k within the chunk, the tile's 64 channels c
      const int rowin = (wave + 4 * j) * 8 + lrow;
      offW[j] = rowin * RSC + a0 + (pc ^ trswz(rowin)) * 8;
    }
  }
  // the loop's tap index is the HALO offset: DGRAD pairs halo offset (r, s) with weight tap (2 - r, 2 - s)
  auto stage_w = [&](char* dst, int cc, int tap) {
    const int wt = PASS == FX_FWD ? tap : 8 - tap;
    const int add = PASS == FX_FWD ? (wt * p.C + cc * 64) : (cc * 64 * RSC + wt * p.C);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
      for (int j = 0; j < NIW; ++j)
        glds16(p.w + pl * p.wstride + offW[j] + add, dst + pl * FX_WBYTES + (wave + 4 * j) * 1024);
  };

  // ---- halo units: unit u of this thread is halo row (u 256 + t) / 8, channels 8 ((u 256 + t) % 8) .. + 7
  const float* const sbase = GEN ? p.src + (size_t)n0 * p.H * p.W * p.Cin : p.src;  // GEN: src_bytes is one image
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)sbase, 0, p.src_bytes, 0x00020000);
  uint32_t hoff[FX_UNITS];  // byte offset of the unit in chunk 0 (DMA_OOB: a padded pixel, loads zeros)
#pragma unroll
  for (int u = 0; u < FX_UNITS; ++u) {
    const int hr = (u * 256 + t) >> 3;
    uint32_t off = DMA_OOB;
    if (GEN && hr < p.nh) {  // halo pixel (hy, hx) of the box around rows y0.., columns q0.. of image n0
      const int hy = (int)fdiv((uint32_t)hr, p.fd_w2), hx = hr - hy * W2;
      const int y = y0 + hy - 1, x = q0 + hx - 1;
      if ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
        off = (uint32_t)(((y * p.W + x) * p.Cin + pc * 8) * 4);
    } else if (hr < p.nh) {
      const int i = hr / p.hb, rem = hr - i * p.hb;
      const int hy = rem / W2, hx = rem - hy * W2;
      const int n = n0 + i, y = y0 + hy - 1, x = hx - 1;
      if (n < p.N && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
        off = (uint32_t)((((n * p.H + y) * p.W + x) * p.Cin + pc * 8) * 4);
    }
    hoff[u] = off;
  }
  f32x4 pf[FX_UNITS][2];  // the next chunk's halo, fp32, in flight / held until the chunk boundary
  auto load_unit = [&](int u, int cc) {
    const uint32_t o = hoff[u] == DMA_OOB ? DMA_OOB : hoff[u] + (uint32_t)(cc * 256);
    f32x_load16(rs, o, pf[u]);
  };
  auto write_halo = [&]() {  // split the held chunk and write its three images
#pragma unroll
    for (int u = 0; u < FX_UNITS; ++u) {
      const int hr = (u * 256 + t) >> 3;
      const float v[8] = {pf[u][0][0], pf[u][0][1], pf[u][0][2], pf[u][0][3],
                          pf[u][1][0], pf[u][1][1], pf[u][1][2], pf[u][1][3]};
      uint4 q0, q1, q2;
      split8(v, q0, q1, q2);
      char* const dst = smem + hr * 128 + ((pc ^ hswz(hr)) << 4);
      *(uint4*)dst = q0;
      *(uint4*)(dst + FX_HBYTES) = q1;
      *(uint4*)(dst + 2 * FX_HBYTES) = q2;
    }
  };

  // ---- B fragments: halo row of each of this lane's pixels at tap (0, 0), then every tap's LDS offset
  const int bcol0 = wave * (FX_BN / 4);
  const int spx = p.rows * p.W;  // pixels per image slice
  const int fpx = GEN ? lane & 15 : fx_frag_pixel(lane & 15, p.W);
  uint32_t boff[9][FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int l = bcol0 + j * 16 + fpx;
    int hbr;
    if constexpr (GEN) {  // (a padded slot's rows run past the box: held within the images' capacity for every tap)
      const int y = (int)fdiv((uint32_t)l, p.fd_segp), x = l - y * p.segp;
      hbr = min(y * W2 + x, FX_HCAP - 1 - 2 * W2 - 2);
    } else {
      const int i = l / spx, rem = l - i * spx;
      const int y = rem / p.W, x = rem - y * p.W;
      hbr = i * p.hb + y * W2 + x;
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) boff[tap][j] = halo_frag_off(hbr + halo_tap_shift<1>(tap, W2, 0), lane);
  }

  // Three accumulator sets. Every MFMA rounds its sum into the accumulator once, so a 9 C / 32 x 6-step chain
  // carries that many roundings at the size of the running sum (measured: 2.9e-7 of sum |x||w| at C = 128, over
  // the bound). acc takes the (0,0) products of ONE chunk (18 steps) and is added into tot by a VALU add at the
  // chunk boundary; lo takes the five correction products, 2^-8 of the sum and so 2^-8 of its roundings.
  f32x4 acc[FM][FN], tot[FM][FN], lo[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = tot[i][j] = lo[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  typedef __attribute__((address_space(3))) bf16x8 lds_bf16x8;
  // one tap: per 32-deep k-step the 3 x (FM + FN) plane fragments, then the six plane products, the smallest
  // first ((0,0) last, into acc); (i, j) innermost, so consecutive MFMAs never share an accumulator
  auto compute = [&](const char* wb, int tap) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 aw[3][FM], bx[3][FN];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
        for (int j = 0; j < FN; ++j)
          bx[pl][j] = *(const lds_bf16x8*)(smem + pl * FX_HBYTES + (boff[tap][j] ^ (uint32_t)(ks * 64)));
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          if constexpr (PASS == FX_FWD) aw[pl][i] = frag_row(wb + pl * FX_WBYTES, i * 16, ks, lane);
          else aw[pl][i] = frag_tr(wb + pl * FX_WBYTES, i * 16, ks, lane);
        }
      }
      constexpr int PW[6] = {2, 1, 0, 1, 0, 0}, PX[6] = {0, 1, 2, 0, 1, 0};  // (weight plane, activation plane)
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            if (q < 5) lo[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[PW[q]][i], bx[PX[q]][j], lo[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[0][i], bx[0][j], acc[i][j], 0, 0, 0);
    }
  };

  // ---- main loop: chunks x 9 unrolled taps. Step (c, tap) reads weight buffer (9 c + tap) & 1; after the step's
  // barrier (every wave is done with the previous step) the next step's weights go to the other buffer and unit
  // `tap` of the next chunk's halo is loaded into registers: both have this tap's MFMAs to land, and the next
  // step's s_waitcnt vmcnt(0) finds them done. At a chunk boundary every wave passes a barrier (the halo images
  // are free), splits its nine held units and writes them; the next step's barrier publishes them.
#pragma unroll
  for (int u = 0; u < FX_UNITS; ++u) load_unit(u, 0);
  stage_w(wbase, 0, 0);
  write_halo();
  for (int c = 0; c < p.nchunk; ++c) {
    const bool more = c + 1 < p.nchunk;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int step = c * 9 + tap;
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      char* const wnext = wbase + ((step + 1) & 1) * FX_WTAP;
      if (tap < 8) stage_w(wnext, c, tap + 1);
      else if (more) stage_w(wnext, c + 1, 0);
      if (more) load_unit(tap, c + 1);
      compute(wbase + (step & 1) * FX_WTAP, tap);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        tot[i][j] += acc[i][j];
        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
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

  // ---- epilogue: D[row = channel a0 + 16 i + 4 (lane >> 4) + v][col = pixel slot bcol0 + 16 j + fpx]
  const int rq = (lane >> 4) * 4;
  float s4[FM][4], q4[FM][4];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int v = 0; v < 4; ++v) s4[i][v] = q4[i][v] = 0.f;
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    size_t pix;
    if constexpr (GEN) {
      const int l = bcol0 + j * 16 + fpx;
      const int y = (int)fdiv((uint32_t)l, p.fd_segp), x = l - y * p.segp;
      if (x >= p.seg || y >= p.rs) continue;  // a padded slot
      pix = ((size_t)n0 * p.H + y0 + y) * p.W + q0 + x;
    } else {
      const int pi = px0 + bcol0 + j * 16 + fpx;
      if (pi >= M) continue;  // a padded image slot of the last tile
      pix = (size_t)pi;
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const size_t o = pix * p.Cout + a0 + i * 16 + rq;
      f32x4 d = tot[i][j] + lo[i][j];
      if constexpr (PASS == FX_DGRAD) {
        if (p.res) d += *(const f32x4*)(p.res + o);
      }
      *(f32x4*)(p.out + o) = d;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        s4[i][v] += d[v];
        q4[i][v] += d[v] * d[v];
      }
    }
  }
  if constexpr (PASS == FX_FWD) {
    if (p.stats != nullptr) {
      float* red = (float*)smem;  // [4][FX_BM][2]
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          s4[i][v] = row16_sum(s4[i][v]);
          q4[i][v] = row16_sum(q4[i][v]);
        }
        if ((lane & 15) == 0) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            red[(wave * FX_BM + i * 16 + rq + v) * 2 + 0] = s4[i][v];
            red[(wave * FX_BM + i * 16 + rq + v) * 2 + 1] = q4[i][v];
          }
        }
      }
      stats_fold<4, FX_BM>(red, p.stats, p.Cout, a0);
    }
  }
  stamp_end(p.ts);
}

// ---------------------------------------------------------------- host side
// Tile geometry of a feasible shape: 128 pixel slots are whole rows of one image or whole images
static bool fx_geometry(const ConvShape& s, TileSplit& t, int& hb, int& nh) {
  if (!conv3x3_ok(s, 1)) return false;
  if (s.W != 4 && s.W != 8 && s.W != 16 && s.W != 32) return false;  // the rows the fragment permutations cover
  if (!classic_tile(s.H, s.W, FX_BN, t)) return false;
  hb = halo_box_s1(t.rows, s.W);
  nh = t.imgs * hb;
  // 32-bit byte offsets of the fp32 tensors (the buffer descriptor's range; DMA_OOB must lie outside it)
  return nh <= FX_HCAP && (uint64_t)s.N * s.H * s.W * std::max(s.C, s.K) * 4 < (1ull << 31);
}

// General geometry of a feasible shape: rs rows x one seg-column segment of one image per tile, every tile row
// padded to segp slots (the kernel's comment); nh halo rows
struct FxGen {
  SegTile g;
  int segp = 0, nh = 0;
};
static bool fx_geometry_gen(const ConvShape& s, FxGen& f) {
  if (!conv3x3_ok(s, 1)) return false;
  const int seg = row_segment(s.W);
  if (seg == 0) return false;
  f.segp = (seg + 15) / 16 * 16;
  f.g = seg_tile(s.H, s.W, seg, rows_dividing(s.H, FX_BN / f.segp));
  f.nh = halo_box_s1(f.g.rs, seg);
  // one image within the per-tile buffer descriptor (32-bit byte offsets; DMA_OOB must lie outside it), and the
  // tile index within FastDiv's 31 bits
  const int64_t cmax = std::max(s.C, s.K);
  return f.nh <= FX_HCAP && (int64_t)s.H * s.W * cmax * 4 < (1ll << 31) &&
         (int64_t)s.N * f.g.tpi * (cmax / FX_BM) < (1ll << 31);
}
// Option f32x_gen: 0 classic geometry only; 1 the general tiles that measured faster than conv_f32;
// 2 every feasible one (for measuring, and the small test shapes)
static bool fx_gen_admitted(const ConvShape& s, const FxGen& f) {
  const int lvl = option_get(OPT_F32X_GEN);
  if (lvl >= 2) return true;
  // measured: tiles of 112 (56- / 28-wide segments) and 98 (14-wide rows) pixels in the 128 slots are
  // 1.5-2.5x faster than conv_f32 at every batch; the 49-pixel tile of 7-wide rows is slower from batch 256 on.
  // Fills between the two were not measured: refused
  return lvl == 1 && f.g.rs * f.g.seg >= 98;
}

bool conv_f32x_ok(const ConvShape& s) {
  TileSplit t;
  int hb, nh;
  if (fx_geometry(s, t, hb, nh)) return true;
  FxGen f;
  return option_get(OPT_F32X_GEN) != 0 && fx_geometry_gen(s, f) && fx_gen_admitted(s, f);
}

int conv_f32x(const ConvShape& s, int mode, const float* src, const u16* wplanes, int64_t wstride, float* out,
              const float* res, int64_t* stats, hipStream_t st, u64* ts) {
  TileSplit t;
  FxGen f;
  int hb = 0, nh = 0;
  DTC_CHECK_ARG(mode == CONV_FWD || mode == CONV_DGRAD, "conv_f32x: forward and data gradient only");
  const bool gen = !fx_geometry(s, t, hb, nh);  // the instance follows the geometry: classic where it holds
  DTC_CHECK_ARG(!gen || fx_geometry_gen(s, f), "conv_f32x: unsupported shape");
  DTC_CHECK_ARG(src && wplanes && out && wstride >= (int64_t)s.K * 9 * s.C && wstride % 8 == 0 &&
                    aligned(wplanes, 16) && aligned(src, 16) && aligned(out, 16) && (!res || aligned(res, 16)),
                "conv_f32x: null / misaligned argument or weight planes closer than one filter bank");
  FxParams p{};
  p.src = src; p.w = wplanes; p.wstride = wstride; p.out = out;
  p.res = mode == CONV_DGRAD ? res : nullptr;
  p.stats = mode == CONV_FWD ? stats : nullptr;
  p.N = s.N; p.H = s.H; p.W = s.W; p.C = s.C;
  p.Cin = mode == CONV_FWD ? s.C : s.K;
  p.Cout = mode == CONV_FWD ? s.K : s.C;
  p.tiles_a = p.Cout / FX_BM;
  p.nchunk = p.Cin / 64;
  p.xcd_remap = option_get(OPT_XCD_REMAP);
  p.ts = ts;
  int64_t tiles_b;
  if (gen) {
    p.src_bytes = (uint32_t)((uint64_t)s.H * s.W * p.Cin * 4);  // one image: the descriptor is made per tile
    p.nh = f.nh;
    p.seg = f.g.seg; p.segp = f.segp; p.rs = f.g.rs; p.spr = f.g.spr; p.tpi = f.g.tpi;
    p.fd_tpi = make_fastdiv(f.g.tpi);
    p.fd_spr = make_fastdiv(f.g.spr);
    p.fd_segp = make_fastdiv(f.segp);
    p.fd_w2 = make_fastdiv(f.g.seg + 2);
    tiles_b = (int64_t)s.N * f.g.tpi;
  } else {
    p.src_bytes = (uint32_t)((uint64_t)s.N * s.H * s.W * p.Cin * 4);
    p.rows = t.rows; p.imgs = t.imgs; p.hb = hb; p.nh = nh;
    p.tiles_y = s.H / t.rows;
    tiles_b = t.imgs == 1 ? s.N * p.tiles_y : (s.N + t.imgs - 1) / t.imgs;
  }
  const dim3 grid((unsigned)(tiles_b * p.tiles_a), 1);
  if (mode == CONV_FWD) {
    if (gen) DTC_KLAUNCH((conv_f32x_kernel<FX_FWD, 1>), grid, dim3(256), 0, st, p);
    else DTC_KLAUNCH((conv_f32x_kernel<FX_FWD, 0>), grid, dim3(256), 0, st, p);
  } else {
    if (gen) DTC_KLAUNCH((conv_f32x_kernel<FX_DGRAD, 1>), grid, dim3(256), 0, st, p);
    else DTC_KLAUNCH((conv_f32x_kernel<FX_DGRAD, 0>), grid, dim3(256), 0, st, p);
  }
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
