// Which kernel a bf16 convolution runs on: the one routing function, and the public launchers that ask it. Every
// family keeps its feasibility predicate beside its kernel; only conv_route knows their order of precedence, the
// slab each pass wants, and the "slab on hand too small" fallbacks. Order (DESIGN.md has the table):
//   FWD    conv_c64 > conv_halo (stride 1, stride 2 column-split) > GEMM
//   DGRAD  conv_c64 > conv_halo (stride 1) > stride-2 classes: dgrad_s2 (no residual) > class GEMM > GEMM
//   WGRAD  wgrad_s2 (one problem, whole dw) > wgrad_halo > GEMM
// Options are read at call time; nothing is cached (tests flip options between calls). conv_launch puts a launcher's
// request, its route and its refusals in one place, for the launchers and for dtc_conv2d_route_query alike.
#include "kernels.h"
#include "tile_common.h"

namespace dtc {

// `splits` equal shares of the reduction steps, none empty
static void set_splits(GemmPlan& g, int splits) {
  g.splits = ceil_div(g.num_kt, ceil_div(g.num_kt, std::max(splits, 1)));
}

static ConvRoute route_wgrad(const ConvShape& s, const ConvRequest& rq) {
  ConvRoute r;
  const int RSC = s.R * s.S * s.C;
  const size_t per_split = (size_t)s.K * RSC * 4;
  r.dw_whole = (rq.dw_cols <= 0 || rq.dw_cols == RSC) && (rq.dw_ld <= 0 || rq.dw_ld == RSC);
  int halo = CONV_K_GEMM;
  if (rq.nprob == 1 && (r.splits = wgrad_s2_splits(s)) > 0) {
    halo = CONV_K_WGRAD_S2;
    r.slab_bytes = conv_wgrad_s2_slab_bytes(s, r.splits);
  } else if ((r.splits = wgrad_halo_splits(s, rq.nprob)) > 0) {
    halo = CONV_K_WGRAD_HALO;
    r.slab_bytes = rq.nprob * r.splits * per_split;
  }
  if (halo == CONV_K_GEMM) {
    r.gemm = igemm_plan(s, CONV_WGRAD, false);
    r.slab_bytes = r.gemm.slab_bytes;
  } else if (rq.slab_bytes >= r.slab_bytes && (halo == CONV_K_WGRAD_HALO || r.dw_whole)) {
    r.kernel = halo;
    r.sc_ok = halo == CONV_K_WGRAD_S2;  // the same launch takes the shortcut's dsc
    return r;
  } else {  // the halo plan's slab is not on hand (or a partial dw at stride 2): 64x64 GEMM tiles, its split count
    const int P = (s.H + 2 * s.pad - s.R) / s.stride + 1, Q = (s.W + 2 * s.pad - s.S) / s.stride + 1;
    r.gemm = GemmPlan{64, 64, r.splits, ceil_div(s.N * P * Q, 64), 0};
  }
  int splits = r.gemm.splits;
  while (splits > 1 && splits * per_split > rq.slab_bytes) --splits;  // as many splits as the slab on hand holds
  set_splits(r.gemm, splits);
  return r;
}

ConvRoute conv_route(const ConvShape& s, int pass, const ConvRequest& rq) {
  if (pass == CONV_WGRAD) return route_wgrad(s, rq);
  ConvRoute r;
  const bool cls = pass == CONV_DGRAD && dgrad_class_mode(s);
  const bool s2 = conv3x3_ok(s, 2);  // conv1 of a projection block: the passes with a shortcut-fused launch
  // the GEMM takes every shape: planned first, its slab wanted whatever runs (the options may change the route)
  r.gemm = igemm_plan(s, pass, cls);
  r.slab_bytes = r.gemm.slab_bytes;
  if (conv_c64_ok(s)) {  // (64 -> 64 channels: one reduction chunk, so conv_halo would want no slab either)
    r.kernel = CONV_K_C64;
    return r;
  }
  r.halo = conv_halo_plan(s, pass);
  if (r.halo.cfg >= 0) {
    r.kernel = CONV_K_HALO;
    const size_t want = conv_halo_slab_bytes(s, pass, r.halo);
    r.slab_bytes = std::max(r.slab_bytes, want);
    if (rq.slab_bytes < want) r.halo.split = 1;
    r.sc_ok = s2;  // (stride 2 is FWD only: the column-split kernel computes the shortcut from the same halo)
    return r;
  }
  if (cls) {  // stride 2, even extents: no split-K
    r.kernel = (rq.sc || !rq.res) && dgrad_s2_halo_ok(s) ? CONV_K_DGRAD_S2 : CONV_K_GEMM_CLASSES;
    r.sc_ok = s2 && option_get(OPT_DGRAD_SCF) != 0;
    return r;
  }
  if (pass == CONV_FWD && s2 && r.gemm.splits == 1) {
    // sc_fuse=1: 64x64-tile plans of at most 512 workgroups (layer4 at B=256: 35.3 us fused vs 8.2 + 31.1
    // separate); 2: every 64x64 plan (layer3: 35.6 vs 9.7 + 23.0 -- the shortcut's own 1024-workgroup launch
    // is cheaper than the fused kernel's lower occupancy); 3: also 128x128 (layer2: its W_sc stage takes
    // LDS to 96 KB, one workgroup per CU: 44.1 vs 11.8 + 21.2)
    const int lvl = option_get(OPT_SC_FUSE);
    const int64_t wgs = (int64_t)(s.K / 64) * ceil_div(s.N * ((s.H + 1) / 2) * ((s.W + 1) / 2), 64);
    r.sc_ok = r.gemm.bn == 64 ? lvl >= 2 || wgs <= 512 : r.gemm.bm != 64 && lvl >= 3;
  }
  if (r.gemm.splits > 1 && rq.slab_bytes < r.gemm.slab_bytes) r.gemm.splits = 1;
  set_splits(r.gemm, r.gemm.splits);
  return r;
}

static ConvRequest with_slab(const float* slab, size_t slab_bytes) {
  ConvRequest rq;
  rq.slab_bytes = slab ? slab_bytes : 0;
  return rq;
}

// The request as the pass's launcher states it, its route, what the launch writes into the slab, and the launcher's
// refusals. The fused FWD launch takes no slab: the statistics and the second output live in the epilogue, so it is
// offered only where the plan is ONE split before any demotion -- conv_route decides sc_ok on the GEMM's planned
// splits, and a split-K plan (a grid too small to fill the chip) is refused, not run on one split; callers then run
// the two convs separately (tests/test_conv_route.py pins this).
ConvLaunch conv_launch(const ConvShape& s, int pass, const ConvRequest& req) {
  ConvLaunch l;
  ConvRequest rq = req;
  if (rq.sc) rq.slab_bytes = pass == CONV_FWD ? 0 : SIZE_MAX;  // (DGRAD: classes or nothing; WGRAD: the launch checks)
  ConvRoute& r = l.route = conv_route(s, pass, rq);
  if (pass != CONV_WGRAD) {
    if (rq.sc && !r.sc_ok) l.refused = pass == CONV_FWD ? "conv_fwd_sc: unsupported shapes" : "conv_dgrad_sc: unsupported geometry / args";
    if (r.kernel == CONV_K_HALO) l.slab_used = conv_halo_slab_bytes(s, pass, r.halo);
    else if (r.kernel == CONV_K_GEMM) l.slab_used = igemm_slab_used(s, pass, r.gemm);
    if (l.refused) l.slab_used = 0;
    return l;
  }
  if (rq.sc) {
    l.slab_used = conv_wgrad_s2_slab_used(s, r.splits);
    if (!r.sc_ok) l.refused = "conv_wgrad_sc: no fused plan for this geometry";
    else if (l.slab_used > req.slab_bytes) l.refused = "conv_wgrad_s2: slab too small";
  } else if (rq.batch) {
    l.slab_used = conv_wgrad_halo_slab_used(s, rq.nprob, r.splits, true);
    if (r.kernel != CONV_K_WGRAD_HALO) l.refused = "conv_wgrad_batch: no halo plan for the problems or slab too small";
  } else if (r.kernel == CONV_K_WGRAD_S2) {
    l.slab_used = conv_wgrad_s2_slab_used(s, r.splits);
  } else {
    if (rq.slab_bytes < (size_t)s.K * s.R * s.S * s.C * 4) l.refused = "wgrad: slab workspace too small";
    l.slab_used = r.kernel == CONV_K_WGRAD_HALO ? conv_wgrad_halo_slab_used(s, 1, r.splits, r.dw_whole)
                                                : igemm_slab_used(s, CONV_WGRAD, r.gemm);
  }
  if (l.refused) l.slab_used = 0;
  return l;
}
#define DTC_LAUNCH_OR_REFUSE(l) \
  if ((l).refused) return set_error(DTC_EINVAL, "%s", (l).refused)

int conv_fwd(const ConvShape& s, const u16* x, const u16* w, u16* y, int64_t* stats, float* slab, size_t slab_bytes,
             hipStream_t st, u64* ts, unsigned* tick) {
  const ConvRoute r = conv_launch(s, CONV_FWD, with_slab(slab, slab_bytes)).route;
  if (r.kernel == CONV_K_C64) return conv_c64(s, CONV_FWD, x, w, y, nullptr, stats, st, ts);
  if (r.kernel == CONV_K_HALO)
    return conv_halo(s, CONV_FWD, r.halo, x, w, y, nullptr, stats, slab, st, ts, nullptr, nullptr, nullptr, tick);
  return igemm_fwd(s, r.gemm, x, w, y, stats, slab, nullptr, nullptr, nullptr, st, ts);
}

// 3x3 stride-2 conv + its block's 1x1 stride-2 projection shortcut in one launch (option sc_fuse): one read of x
static ConvLaunch launch_fwd_sc(const ConvShape& s, const ConvShape& sc) {
  ConvRequest rq;
  rq.sc = true;
  ConvLaunch l = conv_launch(s, CONV_FWD, rq);
  if (!(sc.R == 1 && sc.S == 1 && sc.stride == 2 && sc.pad == 0 && sc.N == s.N && sc.H == s.H && sc.W == s.W &&
        sc.C == s.C && sc.K == s.K))
    l.refused = "conv_fwd_sc: unsupported shapes";
  return l;
}
bool conv_fwd_sc_ok(const ConvShape& s, const ConvShape& sc) { return launch_fwd_sc(s, sc).refused == nullptr; }

int conv_fwd_sc(const ConvShape& s, const ConvShape& sc, const u16* x, const u16* w, u16* y, int64_t* stats,
                const u16* wsc, u16* ysc, int64_t* stats_sc, hipStream_t st, u64* ts) {
  const ConvLaunch l = launch_fwd_sc(s, sc);
  DTC_LAUNCH_OR_REFUSE(l);
  const ConvRoute& r = l.route;
  DTC_CHECK_ARG(x && w && y && wsc && ysc, "conv_fwd_sc: unsupported shapes");
  if (r.kernel == CONV_K_HALO)
    return conv_halo(s, CONV_FWD, r.halo, x, w, y, nullptr, stats, nullptr, st, ts, wsc, ysc, stats_sc);
  return igemm_fwd(s, r.gemm, x, w, y, stats, nullptr, wsc, ysc, stats_sc, st, ts);
}

int conv_dgrad(const ConvShape& s, const u16* dy, const u16* w, u16* dx, const u16* res, float* slab,
               size_t slab_bytes, hipStream_t st, u64* ts, int res_compact, unsigned* tick) {
  ConvRequest rq = with_slab(slab, slab_bytes);
  rq.res = res != nullptr;
  const ConvRoute r = conv_launch(s, CONV_DGRAD, rq).route;
  DTC_CHECK_ARG(!res_compact || (res && r.kernel == CONV_K_GEMM_CLASSES),
                "conv_dgrad: a compact residual needs the stride-2 parity-class path");
  switch (r.kernel) {
    case CONV_K_C64: return conv_c64(s, CONV_DGRAD, dy, w, dx, res, nullptr, st, ts);
    case CONV_K_HALO:
      return conv_halo(s, CONV_DGRAD, r.halo, dy, w, dx, res, nullptr, slab, st, ts, nullptr, nullptr, nullptr, tick);
    case CONV_K_DGRAD_S2: return conv_dgrad_s2_halo(s, dy, w, dx, nullptr, nullptr, st, ts);
    case CONV_K_GEMM_CLASSES:
      return igemm_dgrad(s, r.gemm, true, dy, w, dx, res, res_compact, nullptr, nullptr, nullptr, st, ts);
    default: return igemm_dgrad(s, r.gemm, false, dy, w, dx, res, 0, nullptr, nullptr, slab, st, ts);
  }
}

// conv1 (3x3 stride 2) of a projection block and its 1x1 stride-2 shortcut: dx = dgrad(dc1, W1) + dgrad(dsc, W_sc)
// in ONE launch (the shortcut's term lives at the (even, even) pixels only: no separate shortcut dgrad launch and
// no compact residual pass)
int conv_dgrad_sc(const ConvShape& s, const u16* dy, const u16* w, u16* dx, const u16* dsc, const u16* wsc,
                  hipStream_t st, u64* ts) {
  ConvRequest rq;
  rq.sc = true;
  const ConvLaunch l = conv_launch(s, CONV_DGRAD, rq);
  DTC_LAUNCH_OR_REFUSE(l);
  const ConvRoute& r = l.route;
  DTC_CHECK_ARG(dy && w && dx && dsc && wsc, "conv_dgrad_sc: unsupported geometry / args");
  if (r.kernel == CONV_K_DGRAD_S2) return conv_dgrad_s2_halo(s, dy, w, dx, dsc, wsc, st, ts);
  return igemm_dgrad(s, r.gemm, true, dy, w, dx, nullptr, 0, dsc, wsc, nullptr, st, ts);
}

int conv_wgrad(const ConvShape& s, const u16* x, const u16* dy, float* dw, int dw_cols, int dw_ld, float scale,
               float* slab, size_t slab_bytes, hipStream_t st, u64* ts) {
  ConvRequest rq = with_slab(slab, slab_bytes);
  rq.dw_cols = dw_cols;
  rq.dw_ld = dw_ld;
  const ConvLaunch l = conv_launch(s, CONV_WGRAD, rq);
  DTC_LAUNCH_OR_REFUSE(l);
  const ConvRoute& r = l.route;
  if (r.kernel == CONV_K_WGRAD_S2)
    return conv_wgrad_s2(s, r.splits, x, dy, nullptr, dw, nullptr, scale, slab, slab_bytes, st, ts);
  const int RSC = s.R * s.S * s.C, ncols = dw_cols > 0 ? dw_cols : RSC, ldo = dw_ld > 0 ? dw_ld : RSC;
  int splits = r.gemm.splits;
  if (r.kernel == CONV_K_WGRAD_HALO) {
    DTC_TRY(conv_wgrad_halo(s, 1, &x, &dy, slab, r.splits, &splits, st, ts, r.dw_whole ? &dw : nullptr, scale));
    if (splits == 0) return 0;  // one split: the halo kernel wrote dw itself
  } else {
    DTC_TRY(igemm_wgrad(s, r.gemm, x, dy, slab, st, ts));
  }
  return wgrad_reduce_to(slab, splits, s.K, RSC, ncols, ldo, scale, &dw, 1, st, ts);
}

// conv1's weight gradient and its shortcut's in one launch (wgrad_s2 with dsc); the slab on hand must hold the
// splits that run
int conv_wgrad_sc(const ConvShape& s, const u16* x, const u16* dy, const u16* dsc, float* dw, float* dw_sc, float scale,
                  float* slab, size_t slab_bytes, hipStream_t st, u64* ts) {
  ConvRequest rq = with_slab(slab, slab_bytes);
  rq.sc = true;
  const ConvLaunch l = conv_launch(s, CONV_WGRAD, rq);
  DTC_LAUNCH_OR_REFUSE(l);
  return conv_wgrad_s2(s, l.route.splits, x, dy, dsc, dw, dw_sc, scale, slab, slab ? slab_bytes : 0, st, ts);
}

int conv_wgrad_batch(const ConvShape& s, int nprob, const u16* const* x, const u16* const* dy, float* const* dw,
                     float scale, float* slab, size_t slab_bytes, hipStream_t st, u64* ts) {
  ConvRequest rq = with_slab(slab, slab_bytes);
  rq.nprob = nprob;
  rq.batch = true;
  const ConvLaunch l = conv_launch(s, CONV_WGRAD, rq);
  DTC_LAUNCH_OR_REFUSE(l);
  const ConvRoute& r = l.route;
  int splits = 0;
  DTC_TRY(conv_wgrad_halo(s, nprob, x, dy, slab, r.splits, &splits, st, ts, dw, scale));
  if (splits == 0) return 0;  // one split: the halo kernel wrote dw itself
  const int RSC = s.R * s.S * s.C;
  return wgrad_reduce_to(slab, splits, s.K, RSC, RSC, RSC, scale, dw, nprob, st, ts);
}

}  // namespace dtc
