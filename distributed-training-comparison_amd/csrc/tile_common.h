// Shared by the conv kernels, the one home of the halo family's geometry and layout rules. Host side: the
// classic (whole rows / whole images) and general (row segment) tilings and the halo box sizes; each kernel
// keeps its own limits (halo capacity, 32-bit offsets, its rule for the rows of a general tile) as checks on
// these. Device side (HIP translation units only): LDS-DMA loaders, the LDS swizzles and halo fragment offsets,
// the column-split stride-2 halo, tap shifts, the XCD-grouped workgroup id, the tile origin of the general
// geometry, MFMA fragment readers, the 16-byte epilogue, the BN statistics fold and the call-timing stamps.
#pragma once
#include "common.h"
#include "kernels.h"

namespace dtc {

// ------------------------------------------------------------------ host: the halo planners' tile geometry
// the shape every halo kernel tiles: 3x3, stride st, pad 1, whole 64-channel chunks on both sides
inline bool conv3x3_ok(const ConvShape& s, int st) {
  return s.R == 3 && s.S == 3 && s.stride == st && s.pad == 1 && s.C % 64 == 0 && s.K % 64 == 0;
}
// general geometries, the piece of a w-pixel row per tile row: the row up to 64 pixels, else a dividing segment (or 0)
inline int row_segment(int w) { return w <= 64 ? w : w % 64 == 0 ? 64 : w % 56 == 0 ? 56 : w % 32 == 0 ? 32 : 0; }
// column-split stride-2 halo: LDS row pitch for wo output columns, 2 (wo + 1) [+ 2 where 2 * pitch must be
// 8 mod 16 rows for the tr reads of a 64-pixel step spanning output rows]
inline int s2_pitch(int wo) { return 2 * (wo + 1) + ((wo % 16) == 8 ? 2 : 0); }

// Classic tile: `slots` consecutive positions of an ho x wo grid are slots / wo whole rows of one image
// (imgs = 1), or slots / (ho wo) whole images (rows = ho). False where neither divides.
struct TileSplit {
  int rows = 0, imgs = 0;
};
inline bool classic_tile(int ho, int wo, int slots, TileSplit& t) {
  const int hw = ho * wo;
  if (hw >= slots) {
    if (slots % wo || ho % (slots / wo)) return false;
    t.rows = slots / wo;
    t.imgs = 1;
  } else {
    if (slots % hw) return false;
    t.rows = ho;
    t.imgs = slots / hw;
  }
  return true;
}
// General geometry: a tile is rs rows x one seg-column segment of one image of an ho x wo grid (seg divides wo,
// rs divides ho): spr segments per row, tpi tiles per image. Each kernel chooses seg and rs by its own rule.
struct SegTile {
  int seg = 0, rs = 0, spr = 0, tpi = 0;
};
inline SegTile seg_tile(int ho, int wo, int seg, int rs) { return SegTile{seg, rs, wo / seg, (ho / rs) * (wo / seg)}; }
// the largest row count <= rs that divides h
inline int rows_dividing(int h, int rs) {
  while (rs > 1 && h % rs != 0) --rs;
  return rs;
}
// Halo rows (pixels) of a rows x cols block of positions: the stride-1 box with its one-pixel border, the
// column-split stride-2 input box, and the stride-2 sub-pixel dgrad's dy box (bottom / right neighbours)
inline int halo_box_s1(int rows, int cols) { return (rows + 2) * (cols + 2); }
inline int halo_box_s2(int rows, int cols) { return (2 * rows + 1) * s2_pitch(cols); }
inline int halo_box_subpixel(int rows, int cols) { return (rows + 1) * (cols + 1); }

#ifdef __HIP__
// ------------------------------------------------------------------ device
// LDS-DMA (16 B per lane, lane-linear LDS destination at a wave-uniform base) is issued through
// inline asm on purpose. With the builtins, hipcc treats the DMA as a pending write to LDS and
// emits `s_waitcnt vmcnt(0)` before the next ds_read of ANY LDS buffer, i.e. it drains the
// prefetch of step k+1 before the MFMAs of step k can read their operands (measured in the .s of
// every pipelined kernel here). hipcc neither counts nor waits for an asm DMA: completion is each
// kernel's own counted `s_waitcnt vmcnt(N)` followed by an s_barrier before the data is read.
// M0 (the DMA's LDS base) is compiler-reserved: saved and restored inside the same statement.
__device__ __forceinline__ uint32_t lds_u32(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}

// 16-byte LDS-DMA through a buffer descriptor over [base, base + bytes): an offset outside the
// range loads zeros.
__device__ __forceinline__ void buf_lds16(const void* base, uint32_t bytes, char* lds_dst, uint32_t off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_u32(lds_dst));
  uint32_t keep;
  asm volatile(
      "s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(off), "s"(r), "s"(dst)
      : "memory");
}

// Call-timing stamps (kernel entry / exit only, one lane per workgroup; nothing on the loop).
// Slot layout (u64, one 128-B line per cell): DTC_PROF_LINES start cells, then DTC_PROF_LINES end
// cells. Dispatch order is not guaranteed, so the start is the min over the entries of the first
// DTC_PROF_LINES workgroups (the earliest dispatched among them in practice), each in its own
// line; the end is the max over all workgroups' exits, spread over the end lines. No contention.
__device__ __forceinline__ void stamp_start(u64* ts) {
  if (ts != nullptr && threadIdx.x == 0) {
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (lin < DTC_PROF_LINES) atomicMin(ts + DTC_PROF_LINE * lin, (u64)__builtin_amdgcn_s_memrealtime());
  }
}
__device__ __forceinline__ void stamp_end(u64* ts) {
  if (ts != nullptr && threadIdx.x == 0) {
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    atomicMax(ts + DTC_PROF_LINE * (DTC_PROF_LINES + (lin & (DTC_PROF_LINES - 1))),
              (u64)__builtin_amdgcn_s_memrealtime());
  }
}

// Phase probe (diagnostic builds only: `make phases` -> libdtc_amd_phases.so, -DDTC_PHASES): lane 0 of each
// workgroup writes s_memrealtime (100 MHz, chip-wide) at marked points of a kernel into buf[wg][8]
// (plain vector stores); tools/phase_probe.py reads them. In the product build the marks are empty.
#ifdef DTC_PHASES
constexpr unsigned DTC_PHASE_WGS = 16384;
__device__ __forceinline__ void phase_mark(u64* buf, int k) {
  // wave 0 only, as a wave-uniform branch (a lane-divergent one here would make the compiler treat the
  // buffer descriptors of the surrounding LDS-DMA asm as divergent); its 64 lanes store the same word
  if (buf != nullptr && __builtin_amdgcn_readfirstlane(threadIdx.x) == 0) {
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (lin < DTC_PHASE_WGS) buf[lin * 8 + k] = (u64)__builtin_amdgcn_s_memrealtime();
  }
}
#else
__device__ __forceinline__ void phase_mark(u64*, int) {}
#endif

// Halo LDS swizzle (conv_halo.hip, conv_c64.hip, dgrad_s2.hip): 16-B chunk c of halo row r is stored at chunk c ^ hswz(r).
// Every 8 B-fragment lanes that share a reduction chunk read 8 halo rows that are distinct mod 8 (the per-lane
// pixel order of those kernels guarantees it for W = 4 and 8 too), so (row parity, chunk ^ hswz) spreads them
// over 8 different 16-B bank slots, and the chunk pair (q, q+1) read by one ds_read_b128 lane group lands on
// even / odd slots: conflict-free for EVERY tap shift (rowswz is only for aligned rows).
__device__ __forceinline__ int hswz(int r) { return ((r >> 1) & 3) << 1; }
__device__ __forceinline__ int rowswz(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int trswz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }
// byte offset, within a halo buffer, of the B-fragment chunk (lane >> 4) of halo row `row` (k-step 1: ^ 64)
__device__ __forceinline__ uint32_t halo_frag_off(int row, int lane) {
  return (uint32_t)(row * 128 + (((lane >> 4) ^ hswz(row)) << 4));
}

// A buffer offset no descriptor here covers: the LDS-DMA of it writes zeros, a buffer store of it is dropped.
constexpr uint32_t DMA_OOB = 0x80000000u;

// Column-split stride-2 halo (ST = 2): halo column hx holds column 2 hx of the padded input box (hx < hwh) or
// column 2 (hx - hwh) + 1; -1 past the box's 2 hwh - 1 columns. ST = 1: the halo column itself.
template <int ST>
__device__ __forceinline__ int halo_box_col(int hx, int hwh) {
  return ST == 1 ? hx : (hx < hwh ? 2 * hx : (hx < 2 * hwh - 1 ? 2 * (hx - hwh) + 1 : -1));
}
// halo rows from tap (0, 0) to tap (r, s) = (tap / 3, tap % 3): r row pitches and s columns (column-split: s = 1
// is the first odd column, hwh rows on; s = 2 the next even one)
template <int ST>
__device__ __forceinline__ int halo_tap_shift(int tap, int pitch, int hwh) {
  const int ts = tap % 3;
  return (tap / 3) * pitch + (ST == 1 ? ts : (ts & 1) * hwh + (ts >> 1));
}

// Workgroups go to the 8 XCDs round-robin by linear id: renumber id (of n) so that every XCD owns a contiguous
// range of the new ids, whose neighbours then share an L2.
__device__ __forceinline__ unsigned xcd_grouped_id(unsigned id, unsigned n) {
  const unsigned x8 = id & 7, q = n >> 3, rr = n & 7;  // XCD x8 starts after x8 * q + min(x8, rr) ids
  return x8 * q + min(x8, rr) + (id >> 3);
}

// General geometry (SegTile): image, first row and first column of tile `tile`
__device__ __forceinline__ void seg_tile_origin(int tile, int tpi, const FastDiv& fd_tpi, int spr, const FastDiv& fd_spr,
                                                int rs, int seg, int& n0, int& y0, int& q0) {
  n0 = (int)fdiv((uint32_t)tile, fd_tpi);
  const int rem = tile - n0 * tpi, yb = (int)fdiv((uint32_t)rem, fd_spr);
  y0 = yb * rs;
  q0 = (rem - yb * spr) * seg;
}

// 16-byte epilogue accesses of the 16x16 MFMA layout: lane l holds 4 consecutive channels of a fragment and lane
// l ^ 16 the next four, so one v_permlane16_swap per dword of a fragment pair (2q, 2q + 1) leaves every lane 8
// consecutive channels of one pixel -- one 16-B access per pair instead of two 8-B ones. Both lanes of a swap
// hold the same pixel. The swap is an involution: a 16-B load goes back to the MFMA layout the same way.
__device__ __forceinline__ void swap16(uint32_t& x, uint32_t& y) {  // rows 1 / 3 of x <-> rows 0 / 2 of y
  const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
  x = r[0];
  y = r[1];
}
// this lane's first channel within the 32 channels of a fragment pair
__device__ __forceinline__ int frag_pair_channel(int lane) {
  const int r4 = lane >> 4;
  return (r4 & 1) * 16 + (r4 >> 1) * 8;
}
// the packed bf16 words a[2], b[2] (4 channels each) of fragments 2q, 2q + 1 -> this lane's 8 channels
__device__ __forceinline__ uint4 frag_pair_pack(const uint32_t (&a)[2], const uint32_t (&b)[2]) {
  uint32_t x0 = a[0], x1 = a[1], y0 = b[0], y1 = b[1];
  swap16(x0, y0);
  swap16(x1, y1);
  return uint4{x0, x1, y0, y1};
}
__device__ __forceinline__ void frag_pair_unpack(uint4 v, uint32_t (&a)[2], uint32_t (&b)[2]) {
  uint32_t x0 = v.x, x1 = v.y, y0 = v.z, y1 = v.w;
  swap16(x0, y0);
  swap16(x1, y1);
  a[0] = x0; a[1] = x1;
  b[0] = y0; b[1] = y1;
}

// BN statistics of a forward tile. After its own lane reduction each kernel stages, per wave column w and channel
// ch, the sum at red[(w * BM + ch) * 2] and the sum of squares behind it ([WC][BM][2]); stats_fold then publishes
// the staging (barrier), and thread ch < BM adds the WC partials in wave order (fp32) and
// adds that one partial into the fixed-point slots (common.h: stat_add; exact, flagged if out of range).
template <int WC, int BM>
__device__ __forceinline__ void stats_fold(const float* red, int64_t* stats, int C, int c0) {
  __syncthreads();
  if ((int)threadIdx.x < BM) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int w = 0; w < WC; ++w) {
      s += red[(w * BM + threadIdx.x) * 2 + 0];
      q += red[(w * BM + threadIdx.x) * 2 + 1];
    }
    stat_add(stats, C, c0 + threadIdx.x, s, q);
  }
}

// 16-byte LDS-DMA from a per-lane global address (global_load_lds_dwordx4).
__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_u32(lds_wave_base));
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(g), "s"(dst)
               : "memory");
}

// Row-image fragment: lane holds row (lane&15), reduction chunk (ks*4 + lane>>4).
__device__ __forceinline__ bf16x8 frag_row(const char* region, int row0, int ks, int lane) {
  const int row = row0 + (lane & 15);
  const int ch = (ks * 4 + (lane >> 4)) ^ rowswz(row);
  uint4 v = *(const uint4*)(region + row * 128 + (ch << 4));
  return __builtin_bit_cast(bf16x8, v);
}

// Tr-image fragment: lane holds column (cb + lane&15), reduction rows ks*32 + 8*(lane>>4) + 0..7.
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x8 frag_tr(const char* region, int cb, int ks, int lane) {
  const int img = cb >> 6, cin = cb & 63;
  const int i = lane & 15, q = i >> 2, pp = i & 3, g = lane >> 4;
  const int unit = (cin >> 2) + pp;
  const char* base = region + img * 8192;
  const int kr0 = ks * 32 + g * 8 + q;
  const int kr1 = kr0 + 4;
  const int f0 = (((kr0 >> 1) & 1) << 2) | (((kr0 >> 3) & 1) << 3);
  const int f1 = (((kr1 >> 1) & 1) << 2) | (((kr1 >> 3) & 1) << 3);
  typedef __attribute__((address_space(3))) bf16x4_t lds_v4;
  bf16x4_t t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(base + kr0 * 128 + ((unit ^ f0) << 3)));
  bf16x4_t t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(base + kr1 * 128 + ((unit ^ f1) << 3)));
  return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
}
#endif  // __HIP__

}  // namespace dtc
