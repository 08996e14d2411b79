// Augmentation policies in the on-device CIFAR input launch: RandAugment / TrivialAugmentWide op chains and
// RandomErasing, one launch per batch. Per image:
//   gather -> zero-padded crop -> flip            as cifar_augment_kernel (augment.hip)
//   n_ops policy ops on the uint8 HWC image       in LDS, each reading one buffer and writing the other
//   ToTensor / Normalize                          the same 768-entry table and fp32 operations as augment.hip
//   erase box -> 0.0f                             RandomErasing(value = 0), which is applied after Normalize
// or, with out_u8, the uint8 image before Normalize (the input of a following cifar_augment_mix launch).
// No randomness here: ops, their six fp32 args and the boxes are drawn on the host (data.policy_params /
// data.erase_params), as Mixup / CutMix's parameters are.
//
// Ops (a = current uint8 image, g = the op's args; fp32 expressions evaluated as written, contraction off for
// the whole file; conversions to uint8 clamp to [0, 255], then truncate):
//   0 Identity
//   1 Affine, nearest, fill 0   X = ox + 0.5 - 0.5 w, Y = oy + 0.5 - 0.5 h; sx = (g0 X + g1 Y) + g2,
//                               sy = (g3 X + g4 Y) + g5; rx = rint(sx + (0.5 w - 0.5)), ry likewise with h;
//                               a[ry][rx] when 0 <= rx <= w - 1 and 0 <= ry <= h - 1 (compared as floats), else 0
//   2 Brightness  g0 a + g1 0        3 Color     g0 a + g1 gray, gray = trunc((0.2989 R + 0.587 G) + 0.114 B)
//   4 Contrast    g0 a + g1 m, m = (float)(sum of gray) / (float)(h w)
//   5 Sharpness   g0 a + g1 blur, blur = a on the border, (8 neighbours + 5 centre + 6) / 13 in integers inside
//   6 Posterize   a & (int)g0        7 Solarize  (float)a >= g0 ? 255 - a : a
//   8 AutoContrast per channel: lo == hi ? a : trunc(clamp(((float)a - lo) * (255 / (float)(hi - lo))))
//   9 Equalize per channel: step = (h w - hist[last non-empty bin]) / 255; step == 0 ? a :
//                           min(255, (exclusive_cumsum(hist)[a] + step / 2) / step)
// An op code above 9, a non-finite arg of an op that reads it, a Posterize arg that is no integer in [0, 255]:
// status is set and the op is the Identity. An erase box that is inverted or leaves the image: status, not applied.
//
// One 256-thread workgroup per up to 4 images, as augment.hip. Static LDS, 40,512 B (39.6 KiB) of the 64 KiB a
// workgroup may have:
//   buf   2 x 12 KiB   the images; an op reads an image from one and writes it to the other, per image
//   lut   3 KiB        the normalize table
//   tab   12 KiB       per image 3 x 256 words: Equalize's histogram, then (ops 8 and 9) the byte -> byte table
//   sarg, sop, red     the workgroup's args and validated op codes, and the integer sum / min / max slots
// Images that share a workgroup run different ops and the last workgroup is ragged, so every op is four phases
// that all 256 threads walk through, with the barriers between the phases and never inside a branch:
//   reset (tab of Equalize images, red) | reduce (gray sum, channel min / max, histogram: integer LDS atomics,
//   order-independent) | table (wave q builds image q's byte table) | apply (cur -> other buffer)
// Inside a phase the loop over the workgroup's images is outermost and the op of an image is workgroup-uniform.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace dtc {

constexpr int POL_MAX_BYTES = 12 * 1024;  // one buffer: imgs * h * w * 3 bytes
constexpr int POL_IMGS = 4;               // images per workgroup = waves per workgroup (the table phase)
constexpr int POL_MAX_OPS = 4;

__device__ __forceinline__ uint32_t pol_u8(float s) { return s >= 0.f ? (s <= 255.f ? (uint32_t)(int)s : 255u) : 0u; }

__device__ __forceinline__ uint32_t pol_blend(float g0, uint32_t a, float g1, float b) {
  const float x = g0 * (float)a;
  const float y = g1 * b;
  return pol_u8(x + y);
}

__device__ __forceinline__ uint32_t pol_gray(uint32_t r, uint32_t g, uint32_t b) {
  const float x = 0.2989f * (float)r;
  const float y = 0.587f * (float)g;
  const float z = 0.114f * (float)b;
  return (uint32_t)(int)((x + y) + z);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

__global__ void __launch_bounds__(256) cifar_augment_policy_kernel(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ targets, int64_t n_images,
    const int64_t* __restrict__ index, const uint8_t* __restrict__ crop, const uint8_t* __restrict__ flip, int n,
    int h, int w, int pad, int imgs, float m0, float m1, float m2, float s0, float s1, float s2,
    const uint8_t* __restrict__ ops, const float* __restrict__ args, int n_ops, const uint8_t* __restrict__ erase,
    float* __restrict__ out, uint8_t* __restrict__ out_u8, int64_t* __restrict__ labels, int* __restrict__ status) {
  __shared__ uint32_t buf[2][POL_MAX_BYTES / 4];
  __shared__ float lut[3 * 256];
  __shared__ uint32_t tab[POL_IMGS][3][256];
  __shared__ float sarg[POL_IMGS][POL_MAX_OPS][6];
  __shared__ int sop[POL_IMGS][POL_MAX_OPS];
  __shared__ int red[POL_IMGS][8];  // gray sum, min[3], max[3]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  {
    const float t = (float)tid / 255.0f;
    lut[tid] = (t - m0) / s0;
    lut[256 + tid] = (t - m1) / s1;
    lut[512 + tid] = (t - m2) / s2;
  }
  const int hw = h * w;
  const int ndw = hw * 3 / 4;
  const int b0 = blockIdx.x * imgs;
  const int nb = min(imgs, n - b0);
  // the workgroup's op codes, validated, and args
  if (tid < POL_IMGS * POL_MAX_OPS) {
    const int q = tid / POL_MAX_OPS, k = tid - q * POL_MAX_OPS;
    int op = 0;
    if (q < nb && k < n_ops) {
      const int64_t e = (int64_t)(b0 + q) * n_ops + k;
      op = ops[e];
      float g[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) sarg[q][k][j] = g[j] = args[e * 6 + j];
      const int nargs = op == 1 ? 6 : (op >= 2 && op <= 5) ? 2 : (op == 6 || op == 7) ? 1 : 0;
      bool ok = op <= 9;
#pragma unroll
      for (int j = 0; j < 6; ++j) ok = ok && (j >= nargs || __builtin_isfinite(g[j]));
      if (op == 6) ok = ok && g[0] >= 0.f && g[0] <= 255.f && g[0] == truncf(g[0]);
      if (!ok) {
        op = 0;
        if (status) *status = 1;
      }
    }
    sop[q][k] = op;
  }
  for (int q = 0; q < nb; ++q) {
    const int b = b0 + q;
    const int64_t src = index ? index[b] : (int64_t)b;
    const bool valid = src >= 0 && src < n_images;
    if (tid == 0) {
      if (labels) labels[b] = valid ? targets[src] : 0;
      const int ci = crop ? crop[2 * b] : pad, cj = crop ? crop[2 * b + 1] : pad;
      bool bad = !valid || ci > 2 * pad || cj > 2 * pad;
      if (erase) {
        const int y0 = erase[4 * b], y1 = erase[4 * b + 1], x0 = erase[4 * b + 2], x1 = erase[4 * b + 3];
        bad = bad || !(y0 <= y1 && y1 <= h && x0 <= x1 && x1 <= w);
      }
      if (status && bad) *status = 1;
    }
    const uint32_t* s = (const uint32_t*)(images + (valid ? src : 0) * (int64_t)hw * 3);
    uint32_t* d = buf[0] + q * ndw;
    for (int i = tid; i < ndw; i += 256) d[i] = valid ? s[i] : 0u;
  }
  __syncthreads();
  // crop + flip: buf[0] -> buf[1]
  for (int q = 0; q < nb; ++q) {
    const int b = b0 + q;
    const int ci = crop ? crop[2 * b] : pad;
    const int cj = crop ? crop[2 * b + 1] : pad;
    const bool fl = flip ? flip[b] != 0 : false;
    const uint8_t* px = (const uint8_t*)(buf[0] + q * ndw);
    uint8_t* dst = (uint8_t*)(buf[1] + q * ndw);
    for (int p = tid; p < hw; p += 256) {
      const int oh = p / w, ow = p - oh * w;
      const int y = ci + oh - pad;
      const int x = cj + (fl ? (w - 1 - ow) : ow) - pad;
      const bool in = y >= 0 && y < h && x >= 0 && x < w;
      const uint8_t* sp = px + (in ? (y * w + x) * 3 : 0);
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[p * 3 + c] = in ? sp[c] : (uint8_t)0;
    }
  }
  unsigned sel = (1u << POL_IMGS) - 1;  // bit q: the buffer that holds image q
  __syncthreads();
  const float fw = (float)w, fh = (float)h;
  for (int k = 0; k < n_ops; ++k) {
    // ---- reset
    for (int q = 0; q < nb; ++q)
      if (sop[q][k] == 9)
        for (int i = tid; i < 768; i += 256) (&tab[q][0][0])[i] = 0u;
    if (tid < POL_IMGS * 8) {
      const int j = tid & 7;
      red[tid >> 3][j] = (j >= 1 && j <= 3) ? 255 : 0;
    }
    __syncthreads();
    // ---- reduce
    for (int q = 0; q < nb; ++q) {
      const int op = sop[q][k];
      const uint8_t* a = (const uint8_t*)(buf[(sel >> q) & 1] + q * ndw);
      if (op == 4) {
        int sum = 0;
        for (int p = tid; p < hw; p += 256) sum += (int)pol_gray(a[p * 3], a[p * 3 + 1], a[p * 3 + 2]);
        sum = wave_sum(sum);
        if (lane == 0) atomicAdd(&red[q][0], sum);
      } else if (op == 8) {
        int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
        for (int p = tid; p < hw; p += 256) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int v = a[p * 3 + c];
            lo[c] = min(lo[c], v);
            hi[c] = max(hi[c], v);
          }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int l = wave_min(lo[c]), u = wave_max(hi[c]);
          if (lane == 0) {
            atomicMin(&red[q][1 + c], l);
            atomicMax(&red[q][4 + c], u);
          }
        }
      } else if (op == 9) {
        for (int p = tid; p < hw; p += 256) {
#pragma unroll
          for (int c = 0; c < 3; ++c) atomicAdd(&tab[q][c][a[p * 3 + c]], 1u);
        }
      }
    }
    __syncthreads();
    // ---- table: wave q builds image q's byte table, lane l the bins 4l .. 4l+3
    for (int q = wave; q < nb; q += 4) {
      const int op = sop[q][k];
      if (op == 8) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int lo = red[q][1 + c], hi = red[q][4 + c];
          const float scale = 255.0f / (float)(hi - lo);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int v = 4 * lane + j;
            tab[q][c][v] = lo == hi ? (uint32_t)v : pol_u8(((float)v - (float)lo) * scale);
          }
        }
      } else if (op == 9) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          int hv[4], s = 0, top = -1;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            hv[j] = (int)tab[q][c][4 * lane + j];
            s += hv[j];
            if (hv[j] > 0) top = 4 * lane + j;
          }
          int incl = s;
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
          }
          const int last = max(wave_max(top), 0);  // a bin is non-empty: the image has h*w > 0 pixels
          const int step = (hw - (int)tab[q][c][last]) / 255;
          int cum = incl - s;
          uint32_t o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = step == 0 ? (uint32_t)(4 * lane + j) : (uint32_t)min(255, (cum + step / 2) / max(step, 1));
            cum += hv[j];
          }
          // every lane has read its bins and bin `last` above; the stores follow in program order
#pragma unroll
          for (int j = 0; j < 4; ++j) tab[q][c][4 * lane + j] = o[j];
        }
      }
    }
    __syncthreads();
    // ---- apply: cur -> other
    for (int q = 0; q < nb; ++q) {
      const int op = sop[q][k];
      if (op == 0) continue;
      const int cur = (sel >> q) & 1;
      const uint8_t* a = (const uint8_t*)(buf[cur] + q * ndw);
      uint8_t* d = (uint8_t*)(buf[cur ^ 1] + q * ndw);
      const float* g = sarg[q][k];
      const float g0 = g[0], g1 = g[1];
      switch (op) {
        case 1: {
          const float g2 = g[2], g3 = g[3], g4 = g[4], g5 = g[5];
          const float cx = 0.5f * fw, cy = 0.5f * fh;
          for (int p = tid; p < hw; p += 256) {
            const int oy = p / w, ox = p - oy * w;
            const float X = ((float)ox + 0.5f) - cx;
            const float Y = ((float)oy + 0.5f) - cy;
            const float sx = (g0 * X + g1 * Y) + g2;
            const float sy = (g3 * X + g4 * Y) + g5;
            const float rx = rintf(sx + (cx - 0.5f));
            const float ry = rintf(sy + (cy - 0.5f));
            const bool in = rx >= 0.f && rx <= fw - 1.f && ry >= 0.f && ry <= fh - 1.f;
            const uint8_t* sp = a + (in ? ((int)ry * w + (int)rx) * 3 : 0);
#pragma unroll
            for (int c = 0; c < 3; ++c) d[p * 3 + c] = in ? sp[c] : (uint8_t)0;
          }
          break;
        }
        case 2:
          for (int i = tid; i < hw * 3; i += 256) d[i] = (uint8_t)pol_blend(g0, a[i], g1, 0.f);
          break;
        case 3:
          for (int p = tid; p < hw; p += 256) {
            const uint32_t r = a[p * 3], gg = a[p * 3 + 1], bb = a[p * 3 + 2];
            const float gray = (float)pol_gray(r, gg, bb);
            d[p * 3] = (uint8_t)pol_blend(g0, r, g1, gray);
            d[p * 3 + 1] = (uint8_t)pol_blend(g0, gg, g1, gray);
            d[p * 3 + 2] = (uint8_t)pol_blend(g0, bb, g1, gray);
          }
          break;
        case 4: {
          const float m = (float)red[q][0] / (float)hw;
          for (int i = tid; i < hw * 3; i += 256) d[i] = (uint8_t)pol_blend(g0, a[i], g1, m);
          break;
        }
        case 5:
          for (int p = tid; p < hw; p += 256) {
            const int oy = p / w, ox = p - oy * w;
            const bool inner = oy > 0 && oy < h - 1 && ox > 0 && ox < w - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const uint32_t v = a[p * 3 + c];
              uint32_t blur = v;
              if (inner) {
                uint32_t s = 5u * v + 6u;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                  for (int dx = -1; dx <= 1; ++dx)
                    if (dy != 0 || dx != 0) s += a[(p + dy * w + dx) * 3 + c];
                blur = s / 13u;
              }
              d[p * 3 + c] = (uint8_t)pol_blend(g0, v, g1, (float)blur);
            }
          }
          break;
        case 6: {
          const uint32_t mask = (uint32_t)(int)g0;
          for (int i = tid; i < hw * 3; i += 256) d[i] = (uint8_t)(a[i] & mask);
          break;
        }
        case 7:
          for (int i = tid; i < hw * 3; i += 256) {
            const uint32_t v = a[i];
            d[i] = (uint8_t)((float)v >= g0 ? 255u - v : v);
          }
          break;
        default:  // 8, 9: the byte table
          for (int p = tid; p < hw; p += 256) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[p * 3 + c] = (uint8_t)tab[q][c][a[p * 3 + c]];
          }
          break;
      }
      sel ^= 1u << q;
    }
    __syncthreads();
  }
  if (out_u8) {
    for (int q = 0; q < nb; ++q) {
      const uint32_t* s = buf[(sel >> q) & 1] + q * ndw;
      uint32_t* d = (uint32_t*)(out_u8 + (int64_t)(b0 + q) * hw * 3);
      for (int i = tid; i < ndw; i += 256) d[i] = s[i];
    }
    return;
  }
  const int w4 = w >> 2;
  const int per_c = h * w4;
  const int per_img = 3 * per_c;
  for (int gi = tid; gi < nb * per_img; gi += 256) {
    const int q = gi / per_img;
    const int r0 = gi - q * per_img;
    const int b = b0 + q;
    const uint8_t* px = (const uint8_t*)(buf[(sel >> q) & 1] + q * ndw);
    const int c = r0 / per_c;
    const int rem = r0 - c * per_c;
    const int oh = rem / w4;
    const int ow0 = (rem - oh * w4) * 4;
    const float* tabn = lut + c * 256;
    int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    if (erase) {
      y0 = erase[4 * b], y1 = erase[4 * b + 1], x0 = erase[4 * b + 2], x1 = erase[4 * b + 3];
      if (!(y0 <= y1 && y1 <= h && x0 <= x1 && x1 <= w)) y0 = y1 = 0;
    }
    const bool rowin = oh >= y0 && oh < y1;
    f32x4 v;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ow = ow0 + kk;
      const float t = tabn[px[(oh * w + ow) * 3 + c]];
      v[kk] = (rowin && ow >= x0 && ow < x1) ? 0.0f : t;
    }
    *(f32x4*)(out + (int64_t)b * 3 * hw + (int64_t)c * hw + oh * w + ow0) = v;
  }
}

int cifar_augment_policy(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                         const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                         const float* stdv, const uint8_t* ops, const float* args, int n_ops, const uint8_t* erase,
                         float* out, uint8_t* out_u8, int64_t* labels, int* status, hipStream_t st) {
  DTC_CHECK_ARG(images && mean && stdv && n > 0 && h > 0 && w > 0 && pad >= 0 && n_images > 0,
                "cifar_augment_policy: bad args");
  DTC_CHECK_ARG((out != nullptr) != (out_u8 != nullptr),
                "cifar_augment_policy: exactly one of out (fp32, normalized) and out_u8 (uint8 HWC) must be given");
  DTC_CHECK_ARG(!erase || out, "cifar_augment_policy: erase needs the fp32 output (it zeroes after Normalize)");
  DTC_CHECK_ARG(n_ops >= 0 && n_ops <= POL_MAX_OPS && (n_ops == 0 || (ops && args)),
                "cifar_augment_policy: n_ops=%d must be in [0, %d], with ops and args when > 0", n_ops, POL_MAX_OPS);
  DTC_CHECK_ARG(w % 4 == 0 && (int64_t)h * w * 3 <= POL_MAX_BYTES,
                "cifar_augment_policy: bad shape h=%d w=%d (w %% 4 == 0, h*w*3 <= %d)", h, w, POL_MAX_BYTES);
  DTC_CHECK_ARG(!labels || targets, "cifar_augment_policy: labels requested without targets");
  DTC_CHECK_ARG(stdv[0] != 0.f && stdv[1] != 0.f && stdv[2] != 0.f, "cifar_augment_policy: zero std");
  const int imgs = (int)std::max<int64_t>(1, std::min<int64_t>(POL_IMGS, POL_MAX_BYTES / ((int64_t)h * w * 3)));
  DTC_KLAUNCH(cifar_augment_policy_kernel, dim3((n + imgs - 1) / imgs), dim3(256), 0, st, images, targets, n_images,
              index, crop, flip, n, h, w, pad, imgs, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2], ops, args,
              n_ops, erase, out, out_u8, labels, status);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
