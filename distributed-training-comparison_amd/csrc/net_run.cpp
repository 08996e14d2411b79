// ResNet-18 executor, the run: forward and backward as two calls that enqueue hand-written kernels on one stream.
//
//   forward : stem im2col -> conv(+BN stats) -> BN finalize -> BN+ReLU -> 8 BasicBlocks
//             [conv1 -> bn1+relu -> conv2 -> (shortcut conv) -> bn2 (+bn_sc) + add + relu]
//             -> global avg pool + Linear
//   backward: head -> blocks in reverse [BN2 reduce/finalize/apply -> conv2 wgrad/dgrad ->
//             BN1 ... -> conv1 wgrad/dgrad (+shortcut) with the residual gradient fused into
//             the dgrad epilogue] -> stem BN -> stem wgrad, issuing each gradient bucket's
//             RCCL all-reduce on the communicator's side stream as soon as it is complete.
#include <algorithm>
#include <type_traits>
#include "net.h"

namespace dtc {

// Nd<T>: T as a parameter type that takes no part in template deduction (call sites pass nullptr for an absent tensor)
template <typename T> struct NoDeduce { typedef T type; };
template <typename T> using Nd = typename NoDeduce<T>::type;

// ------------------------------------------------------------------ graph capture helpers
// Process-wide: graph capture (begin_capture .. end_capture) and graph destruction (drop_graphs: a device
// drain + hipGraphExecDestroy) are serialised across host threads. Several executors driven by one thread
// each (the thread-group communicator's W ranks in one process) otherwise capture and drain at the same
// time: a device drain while another thread's stream is capturing crashed the HIP runtime (segfault in
// the first backward of test_gpu_ddp_group's graphs-on case). Capture happens once per executor and
// option epoch, so the lock costs nothing per step; no collective is issued inside a captured region
// (bucket all-reduces run between the replayed segments), so a rank holding it never waits on another.
std::recursive_mutex g_graph_mu;

void drop_graphs(Net& n) {
  GraphState& g = n.graph;
  std::lock_guard<std::recursive_mutex> lk(g_graph_mu);
  // An exec may still be running (the caller's previous step is asynchronous). Round 2 saw a rare
  // crash in a HIP runtime thread (no Python frame) when execs were destroyed right after a device
  // drain and the profiling slots their kernels stamp were freed next (dtc_rn18_profile_end). The
  // slots now live in the workspace (never freed while an exec exists) and an exec is destroyed only
  // after (1) the event recorded behind its LAST launch on the launch stream has completed -- the
  // runtime has retired every command of that launch, in stream order -- and (2) a device drain.
  bool any = false;
  for (auto& set : g.fwd_exec)
    for (auto e : set) any = any || e != nullptr;
  for (auto& v : g.bwd_segs) any = any || !v.empty();
  if (!any) return;
  if (g.launched && g.launch_ev) (void)hipEventSynchronize(g.launch_ev);
  (void)hipDeviceSynchronize();
  for (auto& set : g.fwd_exec)
    for (auto& e : set)
      if (e) {
        (void)hipGraphExecDestroy(e);
        e = nullptr;
      }
  for (auto& v : g.bwd_segs) {
    for (auto& sg : v)
      if (sg.exec) (void)hipGraphExecDestroy(sg.exec);
    v.clear();
  }
  g.launched = false;
}
static int graph_launch(Net& n, hipGraphExec_t ex, hipStream_t st) {
  DTC_HIP(hipGraphLaunch(ex, st));
  // drop_graphs waits on this event (the exec's last launch retired) before destroying an exec
  if (!n.graph.launch_ev) DTC_HIP(hipEventCreateWithFlags(&n.graph.launch_ev, hipEventDisableTiming));
  DTC_HIP(hipEventRecord(n.graph.launch_ev, st));
  n.graph.launched = true;
  return 0;
}
// option graphs: 0 = eager launches, 1 = forward and backward replayed from hipGraphs, 2 = forward only,
// 3 = backward only, 4 (default) = eager launches -- except the backward with a communicator whose bucket
// collectives run on a stream of their own (comm_on_side=0: segment graphs, host-issued collectives between
// them). Measured (tools/bench_ab.sh, one MI355X, images/s): the replayed backward is slower than eager at
// every batch (no communicator: B=256 +4-5% eager (r03), B=64 52.8k -> 59.9k (r04j); with a communicator on
// the weight-gradient stream, loopback r04g / r04h: B=256 116.1k -> 125.9k, 128 78.3k -> 87.7k, 64 49.5k ->
// 57.0k, 32 27.0k -> 31.1k), and since the round-4 host-path changes the replayed forward is no faster
// either (r04s, 3 rounds: B=256 132.5k -> 133.9k eager, B=128 93.0k / 93.2k, B=64 59.9k / 60.2k; r04r: B=32
// 33.9k -> 34.3k, with a communicator 32.3k -> 32.8k): a graph launch's host cost and the ~14 us completion
// gap behind it outweigh the launches it saves (`bwd`: which segment asks; `comm`: it has a communicator)
static bool graphs_on(Net& n, bool bwd, bool comm = false) {
  const int g = option_get(OPT_GRAPHS);
  if (n.capture || n.sync || g == 0 || (g == 2 && bwd) || (g == 3 && !bwd)) return false;
  // an accumulating backward (dtc_rn18_set_grad_accum) runs eagerly and leaves the captured graphs alone: the
  // mode alternates from step to step, and the next plain backward replays what was captured before
  if (bwd && n.accum_mode != DTC_ACCUM_OFF) return false;
  // likewise a backward with gradient compression armed (dtc_rn18_set_grad_compress): its bucket points compress,
  // reduce the staging buffer and decompress, none of which a captured segment holds
  if (bwd && n.compress_mode != DTC_COMPRESS_OFF) return false;
  if (g == 4 && (!bwd || !(comm && option_get(OPT_COMM_ON_SIDE) == 0))) return false;
  if (n.graph.epoch != option_epoch()) {  // options are baked into captured launches
    drop_graphs(n);
    n.graph.epoch = option_epoch();
  }
  return true;
}
static int begin_capture(Net& n) {
  GraphState& g = n.graph;
  g_graph_mu.lock();  // released by the matching end_capture (or here on failure)
  g.cap_locked = true;
  hipError_t e = hipSuccess;
  if (!g.cap_st) e = hipStreamCreateWithFlags(&g.cap_st, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamBeginCapture(g.cap_st, hipStreamCaptureModeRelaxed);
  if (e != hipSuccess) {
    g.cap_locked = false;
    g_graph_mu.unlock();
    return set_error((int)e, "begin capture: %s", hipGetErrorString(e));
  }
  return 0;
}
// Ends the capture on the capture stream (always, also when the captured body failed) and releases the lock
// begin_capture took; *out stays null for an empty capture.
static int end_capture(Net& n, int body_rc, hipGraphExec_t* out) {
  *out = nullptr;
  if (!n.graph.cap_locked)  // begin_capture failed (a segment boundary inside the backward): nothing open
    return body_rc != 0 ? body_rc : set_error(DTC_EINVAL, "end_capture without an open capture");
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(n.graph.cap_st, &g);
  int rc = body_rc;
  if (rc == 0 && e != hipSuccess) rc = set_error((int)e, "hipStreamEndCapture: %s", hipGetErrorString(e));
  if (rc == 0) {
    size_t nodes = 0;
    e = hipGraphGetNodes(g, nullptr, &nodes);
    if (e == hipSuccess && nodes > 0) e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    if (e != hipSuccess) rc = set_error((int)e, "graph instantiate: %s", hipGetErrorString(e));
  }
  if (g) (void)hipGraphDestroy(g);
  n.graph.cap_locked = false;
  g_graph_mu.unlock();
  return rc;
}

// ------------------------------------------------------------------ BN helpers
static bool bn_fused() { return option_get(OPT_BN_FUSED_FIN) != 0; }
// Mask-bit BN backward (option bn_mask, default on): the training forward's fused BN apply also
// writes the ReLU mask of its output as bits, and the backward forms dz = dy * bit where it needs it
// instead of reading the bf16 output (2 B) and storing / re-reading dz (4 B) per element.
static bool bn_mask_on(const Net& n) {
  return !n.f32 && option_get(OPT_BN_MASK) != 0 && bn_fused();
}

// SUM all-reduce of one BN's statistic accumulator (exact int64 fixed point, common.h) on the compute
// stream: the slots are first folded into slot 0 (the others zeroed), so the collective carries the
// header (the non-finite flag) and slot 0, DTC_STAT_HDR + 4*C words, not every slot; integer sums make
// the global totals independent of the ranks' order too. Every apply kernel folds the slots, so after
// this each rank folds the global sums (torch SyncBatchNorm's all-gather of per-rank mean/invstd/count,
// as one reduction; every rank's batch is the same size -- checked by the Python DDP wrapper).
static int sync_bn_sums(Net& n, size_t off, int C, hipStream_t st) {
  DTC_TRY(bn_fold_slots(n.at<int64_t>(off), C, st));
  return comm_allreduce(n.sync, n.mem.ws + off, (size_t)DTC_STAT_HDR + (size_t)4 * C, 2, st);
}

static BnFwdArgs fwd_args(Net& n, BNL& b, int64_t count) {
  BnFwdArgs a;
  a.stats = n.at<int64_t>(b.stats);
  a.count = count;
  a.gamma = n.pf(b.gidx);
  a.beta = n.pf(b.bidx);
  a.rmean = n.mem.bufs + b.rm_off;
  a.rvar = n.mem.bufs + b.rv_off;
  a.nbt = n.mem.nbt ? n.mem.nbt + b.nbt : nullptr;
  a.mean = n.at<float>(b.mean);
  a.invstd = n.at<float>(b.invstd);
  return a;
}
// the unfused coefficient pass: batch statistics (train; also updates the running ones) or running statistics
static int bn_finalize_fwd(Net& n, BNL& b, int64_t count, bool train, hipStream_t st) {
  const BnFwdArgs a = fwd_args(n, b, count);
  float *scale = n.at<float>(b.scale), *shift = n.at<float>(b.shift);
  if (train)
    return bn_fwd_finalize(n.at<int64_t>(b.stats), b.C, count, a.gamma, a.beta, a.rmean, a.rvar, a.nbt, 0.1f, 1e-5f,
                           a.mean, a.invstd, scale, shift, st);
  return bn_eval_coef(b.C, a.gamma, a.beta, a.rmean, a.rvar, 1e-5f, a.mean, a.invstd, scale, shift, st);
}

// BN (+ residual / second BN) + ReLU after the producing conv(s): y = relu(bn(x) [+ x2 | + bn2(x2)]), over bf16
// (T = u16) or fp32 activations. Training uses the fused finalize + apply kernel; the two element types differ
// there on purpose: bf16 honours option bn_fused_fin, writes the ReLU mask bits (bn_mask_on, mask_off != 0) and
// takes a profiling slot of kind 3; fp32 always fuses, writes no bits and takes no slot.
template <typename T>
static int bn_act(Net& n, int mode, BNL& b, const T* x, BNL* b2, const Nd<T>* x2, T* y, int64_t M, bool train,
                  hipStream_t st, size_t mask_off = 0) {
  constexpr bool bf = std::is_same<T, u16>::value;
  if (train && n.sync) {  // SyncBN: global per-channel (sum, sumsq) slots, global element count
    DTC_TRY(sync_bn_sums(n, b.stats, b.C, st));
    if (b2) DTC_TRY(sync_bn_sums(n, b2->stats, b2->C, st));
  }
  const int64_t cnt = train && n.sync ? M * n.sync_world : M;  // elements behind each channel's stats
  if (train && (!bf || bn_fused())) {
    const BnFwdArgs a1 = fwd_args(n, b, cnt);
    const BnFwdArgs a2 = b2 ? fwd_args(n, *b2, cnt) : BnFwdArgs{};
    if constexpr (bf) {
      uint8_t* mask = bn_mask_on(n) && mask_off ? n.at<uint8_t>(mask_off) : nullptr;
      PROF(3, (double)M * b.C * (4.0 + (mode != 1 ? 2.0 : 0.0) + (mask ? 0.125 : 0.0)),
           bn_fin_apply(mode, x, a1, x2, b2 ? &a2 : nullptr, y, M, b.C, st, mask, ts));
      return 0;
    } else {
      return bn_fin_apply(mode, x, a1, x2, b2 ? &a2 : nullptr, y, M, b.C, st);
    }
  }
  if (!n.coef_ready) {
    DTC_TRY(bn_finalize_fwd(n, b, cnt, train, st));
    if (b2) DTC_TRY(bn_finalize_fwd(n, *b2, cnt, train, st));
  }
  const float* s1 = n.at<float>(b.scale);
  const float* h1 = n.at<float>(b.shift);
  if (mode == 1) return bn_apply_relu(x, s1, h1, y, M, b.C, st);
  if (mode == 2) return bn_apply_add_relu(x, s1, h1, x2, y, M, b.C, st);
  return bn_apply_dual_relu(x, s1, h1, x2, n.at<float>(b2->scale), n.at<float>(b2->shift), y, M, b.C, st);
}

// ------------------------------------------------------------------ forward
// the BN statistic slots a training forward's conv accumulates into
static int64_t* stats_if(Net& n, const BNL& b, bool train) { return train ? n.at<int64_t>(b.stats) : nullptr; }

// One timed fp32 conv pass (conv_f32.hip) on the compute stream's slab (a pass's profiling kind is its conv mode;
// flops < 0: the conv's own): y = conv(x, w) (+ BN statistics), dx = conv_transpose(dy, w) (+ res),
// dw[k][0:cols] = gs * sum dy (x) im2col(x)
static int f32_conv(Net& n, int mode, const ConvShape& s, const float* a, const float* b, float* out, const float* res,
                    int64_t* stats, float* dw, int cols, float gs, hipStream_t st, double flops) {
  PROF(mode, flops < 0 ? conv_flops(s) : flops,
       conv_f32(s, mode, a, b, out, res, stats, dw, cols, cols, gs, n.at<float>(n.plan.SLAB), n.plan.slab_bytes, st, ts));
  return 0;
}
static int f32_fwd(Net& n, const ConvShape& s, const float* x, const float* w, float* y, int64_t* stats, hipStream_t st,
                   double flops = -1) {
  return f32_conv(n, CONV_FWD, s, x, w, y, nullptr, stats, nullptr, 0, 0.f, st, flops);
}
static int f32_dgrad(Net& n, const ConvShape& s, const float* dy, const float* w, float* dx, const float* res, hipStream_t st) {
  return f32_conv(n, CONV_DGRAD, s, dy, w, dx, res, nullptr, nullptr, 0, 0.f, st, -1);
}
static int f32_wgrad(Net& n, const ConvShape& s, const float* x, const float* dy, float* dw, float gs, hipStream_t st,
                     int cols = 0, double flops = -1) {
  return f32_conv(n, CONV_WGRAD, s, x, dy, nullptr, nullptr, nullptr, dw, cols, gs, st, flops);
}

// fp32 mode (no autocast): same structure as the bf16 bodies with fp32 activations: f32-MFMA convs
// (conv_f32.hip, BN statistics in the forward epilogue), the fused BN apply kernels on fp32
// tensors (no autocast rounding points), a separate masked BN-backward reduction after each dgrad,
// fp32 head with the fp32 master Linear weights.
static int forward_body_f32(Net& n, float* logits, bool train, hipStream_t st) {
  const Plan& p = n.plan;
  const int64_t M0 = (int64_t)n.B * n.H * n.W;
  n.prof.next = train ? 0 : ProfState::SLOTS;
  DTC_TRY(f32_stem_pack_weight(n.pf(n.stem.pidx), n.at<float>(p.WSTEM), 64, st));
  if (train) DTC_TRY(zero_bytes(n.mem.ws + p.stats_lo, p.stats_hi - p.stats_lo, st));  // + the backward sums
  DTC_TRY(f32_fwd(n, f32_stem_shape(n), n.at<float>(p.X0), n.at<float>(p.WSTEM), n.at<float>(p.C0),
                  stats_if(n, n.bn0, train), st, 2.0 * M0 * 64 * 27));
  DTC_TRY(bn_act(n, 1, n.bn0, n.at<float>(p.C0), nullptr, nullptr, n.at<float>(p.A0), M0, train, st));
  const float* in = n.at<float>(p.A0);
  for (auto& b : n.blocks) {
    const int64_t M = (int64_t)n.B * b.Hout * b.Wout;
    DTC_TRY(f32_fwd(n, b.c1.s, in, n.pf(b.c1.pidx), n.at<float>(b.C1), stats_if(n, b.b1, train), st));
    DTC_TRY(bn_act(n, 1, b.b1, n.at<float>(b.C1), nullptr, nullptr, n.at<float>(b.A1), M, train, st));
    DTC_TRY(f32_fwd(n, b.c2.s, n.at<float>(b.A1), n.pf(b.c2.pidx), n.at<float>(b.C2), stats_if(n, b.b2, train), st));
    if (b.proj) {
      DTC_TRY(f32_fwd(n, b.sc.s, in, n.pf(b.sc.pidx), n.at<float>(b.S), stats_if(n, b.bsc, train), st));
      DTC_TRY(bn_act(n, 3, b.b2, n.at<float>(b.C2), &b.bsc, n.at<float>(b.S), n.at<float>(b.OUT), M, train, st));
    } else {
      DTC_TRY(bn_act(n, 2, b.b2, n.at<float>(b.C2), nullptr, in, n.at<float>(b.OUT), M, train, st));
    }
    in = n.at<float>(b.OUT);
  }
  const BlockL& last = n.blocks.back();
  return head_fwd(in, n.B, last.Hout * last.Wout, 512, n.pf(n.fc_w), n.pf(n.fc_b), n.ncls, n.at<float>(p.FEAT),
                  logits, st);
}

// everything after the input im2col (reads only executor-owned memory: capturable)
static int forward_head(Net& n, float* logits, hipStream_t st) {
  const BlockL& last = n.blocks.back();
  return head_fwd(n.at<u16>(last.OUT), n.B, last.Hout * last.Wout, 512, n.wbf(n.fc_w), n.pf(n.fc_b), n.ncls,
                  n.at<float>(n.plan.FEAT), logits, st);
}

// one timed bf16 forward conv of a block, on the compute stream's slab and split-K counters
static int fwd_conv(Net& n, const ConvShape& s, const u16* x, const u16* w, u16* y, int64_t* stats, hipStream_t st) {
  PROF(0, conv_flops(s), conv_fwd(s, x, w, y, stats, n.at<float>(n.plan.SLAB), n.plan.slab_bytes, st, ts, n.tick(0)));
  return 0;
}
static int forward_body(Net& n, float* logits, bool train, hipStream_t st) {
  if (n.f32) return forward_body_f32(n, logits, train, st);
  const Plan& p = n.plan;
  const int64_t M0 = (int64_t)n.B * n.H * n.W;
  n.prof.next = train ? 0 : ProfState::SLOTS;  // eval passes are not timed
  // the forward statistics AND the backward sums of every BN (the backward that follows this training
  // forward accumulates into zeroed slots; its graph then starts with real work, no memset node) --
  // done by forward()'s input-copy launch on the direct-stem path
  if (train && !p.stem_direct) DTC_TRY(zero_bytes(n.mem.ws + p.stats_lo, p.stats_hi - p.stats_lo, st));
  if (p.stem_direct) {  // stem.hip: taps gathered per tile from the fp32 input, one K=32 k-step
    PROF(0, 2.0 * M0 * 64 * 27,
         stem_fwd(n.at<float>(p.XIN), n.wbf(n.stem.pidx), n.at<u16>(p.C0), stats_if(n, n.bn0, train), n.B, n.H, n.W, st, ts));
  } else {
    DTC_TRY(stem_pack_weight(n.wbf(n.stem.pidx), n.at<u16>(p.WSTEM), 64, st));
    PROF(0, 2.0 * M0 * 64 * 27,
         conv_fwd(n.stem.s, n.at<u16>(p.X0), n.at<u16>(p.WSTEM), n.at<u16>(p.C0),
                  stats_if(n, n.bn0, train), n.at<float>(p.SLAB), p.slab_bytes, st, ts));
  }
  DTC_TRY(bn_act(n, 1, n.bn0, n.at<u16>(p.C0), nullptr, nullptr, n.at<u16>(p.A0), M0, train, st, p.MA0));
  const u16* in = n.at<u16>(p.A0);
  n.side.ev_next = 0;
  for (auto& b : n.blocks) {
    const int64_t M = (int64_t)n.B * b.Hout * b.Wout;
    // option sc_fuse: the projection shortcut inside conv1's launch (its centre-tap im2col tiles)
    const bool scf = b.proj && option_get(OPT_SC_FUSE) != 0 && conv_fwd_sc_ok(b.c1.s, b.sc.s);
    if (b.proj && !scf)  // the shortcut conv first
      DTC_TRY(fwd_conv(n, b.sc.s, in, n.wbf(b.sc.pidx), n.at<u16>(b.S), stats_if(n, b.bsc, train), st));
    if (scf) {
      PROF(0, conv_flops(b.c1.s) + conv_flops(b.sc.s),
           conv_fwd_sc(b.c1.s, b.sc.s, in, n.wbf(b.c1.pidx), n.at<u16>(b.C1), stats_if(n, b.b1, train),
                       n.wbf(b.sc.pidx), n.at<u16>(b.S), stats_if(n, b.bsc, train), st, ts));
    } else {
      DTC_TRY(fwd_conv(n, b.c1.s, in, n.wbf(b.c1.pidx), n.at<u16>(b.C1), stats_if(n, b.b1, train), st));
    }
    DTC_TRY(bn_act(n, 1, b.b1, n.at<u16>(b.C1), nullptr, nullptr, n.at<u16>(b.A1), M, train, st, b.MA1));
    DTC_TRY(fwd_conv(n, b.c2.s, n.at<u16>(b.A1), n.wbf(b.c2.pidx), n.at<u16>(b.C2), stats_if(n, b.b2, train), st));
    if (b.proj) {
      DTC_TRY(bn_act(n, 3, b.b2, n.at<u16>(b.C2), &b.bsc, n.at<u16>(b.S), n.at<u16>(b.OUT), M, train, st, b.MOUT));
    } else {
      DTC_TRY(bn_act(n, 2, b.b2, n.at<u16>(b.C2), nullptr, in, n.at<u16>(b.OUT), M, train, st, b.MOUT));
    }
    in = n.at<u16>(b.OUT);
  }
  // graphed forward: the head is launched by forward() after the graph, into the caller's logits
  if (logits == nullptr) return 0;
  return forward_head(n, logits, st);
}

static int forward(Net& n, const float* x, float* logits, bool train, hipStream_t st) {
  const Plan& p = n.plan;
  n.prof.st = st;
  // graphed bf16 forward: the pool + FC head is launched after the graph straight into the caller's logits
  // (the graph cannot bake in a per-call pointer); the fp32 executor's graph writes a graph-owned buffer
  // that is copied out after the replay
  if (n.f32) DTC_TRY(f32_stem_im2col(x, n.at<float>(p.X0), n.B, n.H, n.W, st));
  else if (p.stem_direct) {  // the graph reads only executor memory: a copy of the 12 B/pixel input (+ the
    // training step's BN slots zeroed in the same launch)
    const size_t xb = (size_t)n.B * 3 * n.H * n.W * 4;
    if (xb % 16 == 0 && ((uintptr_t)x & 15) == 0 && option_get(OPT_STEM_PROLOGUE) != 0) {
      DTC_TRY(copy_and_zero(x, n.at<float>(p.XIN), xb, n.mem.ws + p.stats_lo, train ? p.stats_hi - p.stats_lo : 0, st));
    } else {
      DTC_HIP(hipMemcpyAsync(n.at<float>(p.XIN), x, xb, hipMemcpyDeviceToDevice, st));
      if (train) DTC_TRY(zero_bytes(n.mem.ws + p.stats_lo, p.stats_hi - p.stats_lo, st));
    }
  } else {
    DTC_TRY(stem_im2col(x, n.at<u16>(p.X0), n.B, n.H, n.W, st));
  }
  if (!graphs_on(n, false)) return forward_body(n, logits, train, st);
  hipGraphExec_t& ex = n.graph.fwd_exec[n.prof.on ? 1 : 0][train ? 1 : 0];
  if (!ex) {
    DTC_TRY(begin_capture(n));
    const int rc = forward_body(n, n.f32 ? n.at<float>(p.LOGITS) : nullptr, train, n.graph.cap_st);
    DTC_TRY(end_capture(n, rc, &ex));
  }
  DTC_TRY(graph_launch(n, ex, st));
  if (!n.f32) return forward_head(n, logits, st);
  DTC_HIP(hipMemcpyAsync(logits, n.at<float>(p.LOGITS), (size_t)n.B * n.ncls * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

// One evaluation batch (reference trainer.py validate / test): the eval-mode forward of the first nv images of
// x and the batch's metrics, enqueued with no host synchronisation. The input is staged as forward stages
// it, for nv images, and the remaining B - nv image slots of the executor's own input are zeroed: eval-mode rows
// are independent (running statistics), so the valid rows' logits do not depend on the padding, and a short
// last batch needs no second executor. Every BN's coefficients come from ONE launch (bn_eval_coef_all) instead
// of one per BN; the body then runs as forward(train = 0) does, always eagerly (no graph is captured, replayed
// or dropped) and without profiling slots.
static int eval_batch(Net& n, const float* x, const int64_t* labels, int nv, int topk, float* logits,
                      ::dtc_eval_record* rec, hipStream_t st) {
  const Plan& p = n.plan;
  n.prof.st = st;
  const size_t img = (size_t)n.H * n.W;  // pixels per image
  const int pad = n.B - nv;
  if (n.f32) {  // fp32 im2col rows [B*H*W][32]
    DTC_TRY(f32_stem_im2col(x, n.at<float>(p.X0), nv, n.H, n.W, st));
    if (pad) DTC_TRY(zero_bytes(n.mem.ws + p.X0 + (size_t)nv * img * 32 * 4, (size_t)pad * img * 32 * 4, st));
  } else if (p.stem_direct) {  // the executor's copy of the fp32 NCHW input
    const size_t xb = (size_t)nv * 3 * img * 4, zb = (size_t)pad * 3 * img * 4;
    char* xin = n.mem.ws + p.XIN;
    if (xb % 16 == 0 && zb % 8 == 0 && ((uintptr_t)x & 15) == 0 && option_get(OPT_STEM_PROLOGUE) != 0) {
      DTC_TRY(copy_and_zero(x, xin, xb, xin + xb, zb, st));  // one launch: copy the images, zero the padding
    } else {
      DTC_HIP(hipMemcpyAsync(xin, x, xb, hipMemcpyDeviceToDevice, st));
      if (zb) DTC_HIP(hipMemsetAsync(xin + xb, 0, zb, st));
    }
  } else {  // bf16 im2col rows [B*H*W][64]
    DTC_TRY(stem_im2col(x, n.at<u16>(p.X0), nv, n.H, n.W, st));
    if (pad) DTC_TRY(zero_bytes(n.mem.ws + p.X0 + (size_t)nv * img * 64 * 2, (size_t)pad * img * 64 * 2, st));
  }
  BnEvalTable tab;
  DTC_CHECK_ARG(n.bns.size() <= (size_t)DTC_EVAL_BN_MAX, "eval_batch: %zu BatchNorms", n.bns.size());
  for (BNL* b : n.bns) {
    BnEvalEntry& e = tab.e[tab.n++];
    e.C = b->C;
    e.gamma = n.pf(b->gidx);
    e.beta = n.pf(b->bidx);
    e.rmean = n.mem.bufs + b->rm_off;
    e.rvar = n.mem.bufs + b->rv_off;
    e.mean = n.at<float>(b->mean);
    e.invstd = n.at<float>(b->invstd);
    e.scale = n.at<float>(b->scale);
    e.shift = n.at<float>(b->shift);
  }
  DTC_TRY(bn_eval_coef_all(tab, 1e-5f, st));
  float* lg = logits ? logits : n.at<float>(p.LOGITS);
  n.coef_ready = true;
  const int rc = forward_body(n, lg, false, st);  // (sets prof.next = SLOTS: eval passes are not timed)
  n.coef_ready = false;
  n.sums_fresh = false;  // the saved mean / invstd slots now hold the running statistics
  DTC_TRY(rc);
  return eval_metrics(lg, labels, nv, n.ncls, topk, rec, st);
}

// ------------------------------------------------------------------ side stream
// Side stream for the weight gradients (fork after their input gradient exists, join before
// anything reads the weight gradients: bucket all-reduces and the end of backward).
static int next_event(Net& n, hipEvent_t* ev) {
  SideState& s = n.side;
  if (s.evs.empty()) {
    s.evs.resize(64);
    for (auto& e : s.evs) DTC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  *ev = s.evs[s.ev_next];
  s.ev_next = (s.ev_next + 1) % (int)s.evs.size();
  return 0;
}
// A marker recorded on `st` (the fork / join points of the weight-gradient stream). Round 6 measured the
// alternative -- waiting on the producing kernel's own stop event (hipExtLaunchKernelGGL) instead of a recorded
// marker, which removes the marker's ~2.7 us bubble in isolation (tools/probes/fork_gap.hip) -- and removed it:
// on a busy stream each such launch cost the host ~4 us and left a ~4.7 us gap after the kernel (B=256 -2.7%,
// 24 of 24 in-process A/B rounds; backward host issue 189 -> 321 us; profiles/r06w_fork_ev.txt)
static int stop_or_record(Net& n, hipStream_t st, hipEvent_t* ev) {
  DTC_TRY(next_event(n, ev));
  DTC_HIP(hipEventRecord(*ev, st));
  return 0;
}
// the side stream waits for everything issued on `st` so far
static int side_wait(Net& n, hipStream_t st) {
  hipEvent_t ev;
  DTC_TRY(stop_or_record(n, st, &ev));
  DTC_HIP(hipStreamWaitEvent(n.side.st, ev, 0));
  g_fork_watch = ForkWatch{st, false};
  return 0;
}
static int fork_side(Net& n, hipStream_t st, hipStream_t* out) {
  if (!side_on()) {
    *out = st;
    return 0;
  }
  if (!n.side.st) {
    // option side_prio: the weight-gradient stream at the lowest priority, so the dispatcher prefers the
    // dgrad / BN chain (the critical path) when both have workgroups ready
    if (option_get(OPT_SIDE_PRIO) != 0) {
      int lo = 0, hi = 0;
      DTC_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo = least urgent
      DTC_HIP(hipStreamCreateWithPriority(&n.side.st, hipStreamNonBlocking, lo));
    } else {
      DTC_HIP(hipStreamCreateWithFlags(&n.side.st, hipStreamNonBlocking));
    }
  }
  DTC_TRY(side_wait(n, st));
  n.side.pending = true;
  *out = n.side.st;
  return 0;
}
// the side stream already waits for everything issued on st (forked from it, nothing launched on st since)
static bool side_covers(hipStream_t st) { return g_fork_watch.st == st && !g_fork_watch.dirty; }
static int join_side(Net& n, hipStream_t st) {
  if (!n.side.pending) return 0;
  hipEvent_t ev;
  DTC_TRY(stop_or_record(n, n.side.st, &ev));
  DTC_HIP(hipStreamWaitEvent(st, ev, 0));
  n.side.pending = false;
  return 0;
}

// ------------------------------------------------------------------ deferred weight gradients
// Deferred 3x3 stride-1 weight gradients (option wgrad_batch): every wgrad of the halo geometry is
// queued and issued together with the others of its geometry -- at most wgrad_batch per launch --
// when the geometry changes, before a DDP bucket that needs them is all-reduced, and at the end of
// backward. The inputs stay valid while queued (per-block conv-output gradient buffers, forward
// activations). One batched launch of P problems writes the split-K slab of ONE (conv_wgrad_batch).
struct WgQueue {
  ConvShape s{};
  int count = 0;
  const u16* x[DTC_WG_BATCH] = {};
  const u16* dy[DTC_WG_BATCH] = {};
  float* dw[DTC_WG_BATCH] = {};
};
static int wgrad_batch_max() { return std::min(std::max(option_get(OPT_WGRAD_BATCH), 1), DTC_WG_BATCH); }
static bool same_shape(const ConvShape& a, const ConvShape& b) {
  return a.N == b.N && a.H == b.H && a.W == b.W && a.C == b.C && a.K == b.K && a.R == b.R && a.S == b.S &&
         a.stride == b.stride && a.pad == b.pad;
}
static int wg_flush(Net& n, WgQueue& q, float gs, float* slabw, hipStream_t sd) {
  if (q.count == 0) return 0;
  const int np = q.count;
  q.count = 0;
  PROF(2, conv_flops(q.s) * np,
       np == 1 ? conv_wgrad(q.s, q.x[0], q.dy[0], q.dw[0], 0, 0, gs, slabw, n.plan.slab_bytes, sd, ts)
               : conv_wgrad_batch(q.s, np, q.x, q.dy, q.dw, gs, slabw, n.plan.slab_bytes, sd, ts));
  return 0;
}
// the flush at a bucket point and before the stem: with option fork_lazy the side stream is forked here,
// and only when the queue holds something to launch
static int wg_flush_forked(Net& n, WgQueue& q, float gs, float* slabw, hipStream_t& sd, hipStream_t st) {
  if (option_get(OPT_FORK_LAZY) != 0 && q.count > 0) DTC_TRY(fork_side(n, st, &sd));
  return wg_flush(n, q, gs, slabw, sd);
}
// lazy (option fork_lazy): the side stream is forked from `st` here, only when something is launched,
// instead of by the caller before every wgrad (a queued-only wgrad needs no fork: the launch's fork
// is later on the main stream, so it covers the queued inputs too)
static int wg_issue(Net& n, WgQueue& q, const ConvShape& s, const u16* x, const u16* dy, float* dw, float gs,
                    float* slabw, hipStream_t& sd, hipStream_t st = nullptr, bool lazy = false) {
  const int bmax = wgrad_batch_max();
  ConvRequest two;
  two.nprob = 2;
  if (bmax <= 1 || conv_route(s, CONV_WGRAD, two).kernel != CONV_K_WGRAD_HALO) {  // no batched launch for s
    if (lazy) DTC_TRY(fork_side(n, st, &sd));
    PROF(2, conv_flops(s), conv_wgrad(s, x, dy, dw, 0, 0, gs, slabw, n.plan.slab_bytes, sd, ts));
    return 0;
  }
  if (q.count > 0 && !same_shape(q.s, s)) {
    if (lazy) DTC_TRY(fork_side(n, st, &sd));
    DTC_TRY(wg_flush(n, q, gs, slabw, sd));
  }
  q.s = s;
  q.x[q.count] = x;
  q.dy[q.count] = dy;
  q.dw[q.count] = dw;
  if (++q.count >= bmax) {
    if (lazy) DTC_TRY(fork_side(n, st, &sd));
    DTC_TRY(wg_flush(n, q, gs, slabw, sd));
  }
  return 0;
}

// ------------------------------------------------------------------ bucket points
struct BwdCtx {
  Comm* comm = nullptr;
  bool capturing = false;
  std::vector<Seg>* segs = nullptr;
};
// (the plan's bucket points, with or without a communicator: the batches -- and so the split-K
// summation order -- are the same whether or not the gradients are all-reduced)
static bool bucket_fires(const Net& n, int after_block) {
  for (int a : n.plan.bucket_after_block)
    if (a == after_block) return true;
  return false;
}
// Bucket i's all-reduce, bracketed by the timed step's events: on `stream` itself (on_stream: its producers
// are already ordered before it there) or on the communicator's own stream, forked from `stream`. `compressed`
// (gradient compression, the caller has filled the bucket's staging range): the collective reduces the bf16
// staging words, and the decompress into the fp32 gradients is enqueued directly behind it on the stream the
// collective runs on -- outside the timing events, and ahead of the end-of-backward join of that stream.
static int issue_bucket(Net& n, Comm* comm, int i, hipStream_t stream, bool on_stream, bool compressed = false) {
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (n.ct.cur && i < (int)n.ct.cur->b0.size()) {
    t0 = n.ct.cur->b0[i];
    t1 = n.ct.cur->b1[i];
    n.ct.cur->bucket[i] = true;
  }
  float* g = n.mem.g + n.plan.bucket_off[i];
  const size_t len = (size_t)n.plan.bucket_len[i];
  if (!compressed)
    return on_stream ? comm_allreduce_on(comm, g, len, 0, stream, t0, t1)
                     : comm_allreduce_async(comm, g, len, 0, stream, t0, t1);
  u16* c = n.compress + n.plan.bucket_off[i];
  DTC_TRY(on_stream ? comm_allreduce_on(comm, c, len, 1, stream, t0, t1)
                    : comm_allreduce_async(comm, c, len, 1, stream, t0, t1));
  return grad_decompress_bf16(c, g, (int64_t)len, on_stream ? stream : comm_side_stream(comm));
}
// Bucket point after block `after_block` (-1: after the stem). Eager: all-reduce the buckets that
// are complete now. Capturing: close the current graph segment there and open the next one; the
// replay issues the all-reduces between segments.
static int maybe_bucket(Net& n, int after_block, const BwdCtx& cx, hipStream_t st) {
  const int accum = n.accum_mode;
  if (!cx.comm && accum == DTC_ACCUM_OFF) return 0;
  std::vector<int> ids;
  for (size_t i = 0; i < n.plan.bucket_off.size(); ++i)
    if (n.plan.bucket_after_block[i] == after_block) ids.push_back((int)i);
  if (ids.empty()) return 0;
  if (!cx.capturing) {
    // The bucket's producers are the compute stream (BN dgamma / dbeta, the head) and the weight-gradient
    // side stream. The compute stream does NOT wait for the side stream here (that join would stall the
    // dgrad / BN chain behind the queued weight gradients at every bucket point): the side stream is
    // forked from the compute stream instead, so it holds both producers, and the collective is ordered
    // after it. The side stream is joined into the compute stream once, at the end of the backward.
    hipStream_t prod = st;
    if (n.side.pending) {
      // (a flush's fork right before this point already ordered it: no second marker)
      if (!side_covers(st)) DTC_TRY(side_wait(n, st));
      prod = n.side.st;
    }
    // Gradient accumulation (dtc_rn18_set_grad_accum): one launch over the contiguous range of the buckets
    // complete here, on the stream that holds both producers, so it overlaps the rest of the backward as the
    // collective does. STORE / ADD keep the sum in n.accum and reduce nothing (the entry points refuse a
    // communicator); FINISH adds the sum onto the gradients ahead of the buckets' collectives below, which are
    // ordered after `prod`.
    // Gradient compression (dtc_rn18_set_grad_compress; only with a communicator): one compress launch over the
    // same range into the bf16 staging buffer, on `prod` too. With FINISH it is the fused form, staging =
    // bf16(g + acc), in place of the FINISH launch: g + acc is not written to g, the decompress behind each
    // bucket's collective (issue_bucket) overwrites g anyway.
    const bool compress = cx.comm && n.compress_mode == DTC_COMPRESS_BF16;
    if (accum != DTC_ACCUM_OFF || compress) {
      int64_t lo = n.plan.bucket_off[ids[0]], hi = lo;
      for (int i : ids) {
        lo = std::min(lo, n.plan.bucket_off[i]);
        hi = std::max(hi, n.plan.bucket_off[i] + n.plan.bucket_len[i]);
      }
      if (compress)
        DTC_TRY(grad_compress_bf16(n.mem.g + lo, accum == DTC_ACCUM_FINISH ? n.accum + lo : nullptr, n.compress + lo,
                                   hi - lo, prod));
      else
        DTC_TRY(grad_accum(n.accum + lo, n.mem.g + lo, hi - lo, accum, prod));
      if (!cx.comm) return 0;
    }
    // option comm_on_side: the collective on the weight-gradient stream itself (it holds both producers
    // now; the stream is joined into the compute stream at the end of the backward) -- one HIP stream
    // fewer competing for the process's hardware queues (GPU_MAX_HW_QUEUES); the weight gradients of
    // later buckets then queue behind it on that stream
    const bool on_side = option_get(OPT_COMM_ON_SIDE) != 0 && prod == n.side.st;
    // option comm_tail_inline: the last bucket (after the stem, nothing left to overlap) is all-reduced on the
    // compute stream itself when every earlier collective is already ordered before that stream (none
    // pending on the communicator's stream): the fork to the communicator's stream and the join back cost
    // two cross-stream hand-offs, ~15 us each (bench --sim-world 2 buckets_us / comm_exposed_us, round 5)
    const bool inline_tail = after_block == -1 && prod == st && option_get(OPT_COMM_TAIL_INLINE) != 0 &&
                             !comm_pending(cx.comm);
    for (int i : ids) DTC_TRY(issue_bucket(n, cx.comm, i, prod, on_side || inline_tail, compress));
    return 0;
  }
  DTC_TRY(join_side(n, st));  // a graph segment ends here: every stream forked in it joins back
  Seg sg;
  sg.buckets = ids;
  DTC_TRY(end_capture(n, 0, &sg.exec));
  cx.segs->push_back(sg);
  return begin_capture(n);
}

// ------------------------------------------------------------------ backward helpers
// Parity captures (n.capture): `src` copied into the slot `name`; the mask-bit backward, which never stores dz,
// materialises it there with bn_mask_apply (cap_masked).
static int cap_slot(Net& n, const std::string& name, const Act** slot) {
  for (const auto& a : n.plan.caps)
    if (a.name == name) return *slot = &a, 0;
  return set_error(DTC_EINVAL, "capture slot %s missing", name.c_str());
}
static int cap(Net& n, const std::string& name, const void* src, hipStream_t st) {
  if (!n.capture) return 0;
  const Act* a;
  DTC_TRY(cap_slot(n, name, &a));
  DTC_HIP(hipMemcpyAsync(n.mem.ws + a->off, src, (size_t)a->n * a->h * a->w * a->c * n.esz(), hipMemcpyDeviceToDevice, st));
  return 0;
}
static int cap_masked(Net& n, const std::string& name, const u16* dy, size_t mask_off, int64_t M, int C, hipStream_t st) {
  if (!n.capture) return 0;
  const Act* a;
  DTC_TRY(cap_slot(n, name, &a));
  return bn_mask_apply(dy, n.at<uint8_t>(mask_off), (u16*)(n.mem.ws + a->off), M, C, st);
}
// capture-slot prefix of block bi (empty, and no allocation, without captures)
static std::string cap_prefix(const Net& n, int bi) { return n.capture ? "grad." + block_name(bi) : std::string(); }

static BnBwdArgs bwd_args(Net& n, BNL& b, int64_t count, float gs) {
  return BnBwdArgs{n.at<int64_t>(b.acc), count, n.pf(b.gidx), n.at<float>(b.mean), n.at<float>(b.invstd), gs,
                   n.gf(b.gidx), n.gf(b.bidx)};
}

// BN-backward reduction of the BN(s) whose post-ReLU output is `y`: b1 over x1 and, sharing dz, b2 over x2 (the
// projection shortcut's BN). `y` is the output itself or (bits) the forward's ReLU mask bits of it. The bundle
// (kernels.h) is what the reduction passes below take; BnbArgsF32 is its fp32-activation sibling.
struct BnbArgsF32 {
  const float *ym = nullptr, *x1 = nullptr, *mean1 = nullptr, *invstd1 = nullptr;
  int64_t* acc1 = nullptr;
  const float *x2 = nullptr, *mean2 = nullptr, *invstd2 = nullptr;
  int64_t* acc2 = nullptr;
};
template <typename T, typename A>
static void bnb_fill(Net& n, A& a, size_t x1, BNL& b1, size_t x2, BNL* b2) {
  a.x1 = n.at<T>(x1);
  a.mean1 = n.at<float>(b1.mean);
  a.invstd1 = n.at<float>(b1.invstd);
  a.acc1 = n.at<int64_t>(b1.acc);
  if (b2 != nullptr) {
    a.x2 = n.at<T>(x2);
    a.mean2 = n.at<float>(b2->mean);
    a.invstd2 = n.at<float>(b2->invstd);
    a.acc2 = n.at<int64_t>(b2->acc);
  }
}
static BnbArgs bnb_of(Net& n, size_t y, size_t x1, BNL& b1, size_t x2 = 0, BNL* b2 = nullptr, bool bits = false) {
  BnbArgs a;
  if (bits) a.mb = n.at<uint8_t>(y);
  else a.ym = n.at<u16>(y);
  bnb_fill<u16>(n, a, x1, b1, x2, b2);
  return a;
}
static BnbArgsF32 bnb_of_f32(Net& n, size_t y, size_t x1, BNL& b1, size_t x2 = 0, BNL* b2 = nullptr) {
  BnbArgsF32 a;
  a.ym = n.at<float>(y);
  bnb_fill<float>(n, a, x1, b1, x2, b2);
  return a;
}
// the BN(s) behind a block's output: bn2 (+ the projection BN)
static BnbArgs bnb_out(Net& n, BlockL& b, bool bits = false) {
  return bnb_of(n, bits ? b.MOUT : b.OUT, b.C2, b.b2, b.proj ? b.S : 0, b.proj ? &b.bsc : nullptr, bits);
}
// the reduction passes over a bundle: dz = dy * [y > 0] stored (may alias dy) and the sums accumulated ...
template <typename T, typename A>
static int bn_reduce(const A& a, const T* dy, T* dz, int64_t M, int C, hipStream_t st) {
  return bn_bwd_reduce(dy, a.ym, a.x1, a.mean1, a.invstd1, a.acc1, a.x2, a.mean2, a.invstd2, a.acc2, dz, M, C, st);
}
// ... or, from the mask bits, the sums alone (4.125 B/element read, + 2 B for a second BN's input)
static int bn_reduce_mask(Net& n, const BnbArgs& a, const u16* dy, int64_t M, int C, hipStream_t st) {
  PROF(3, (double)M * C * (a.x2 ? 6.125 : 4.125),
       bn_bwd_reduce_mask(dy, a.mb, a.x1, a.mean1, a.invstd1, a.acc1, a.x2, a.mean2, a.invstd2, a.acc2, M, C, st, ts));
  return 0;
}

// Small tensors (option bn_cg, bn_bwd_cg_ok): the mask-bit BN backward -- reduction, coefficients, apply --
// as ONE launch (bn.hip bn_bwd_cg: one workgroup per 8 channels over the whole batch, no statistic slots); not
// with SyncBN (its sums are all-reduced between the two passes)
// Measured (kernel trace r04e, batch 256): at layer4's 4096 x 512 the one launch took 26-30 us against
// 11 us for the pair -- 64 workgroups of 16-B pieces strided by the channel count -- so it is used only
// for tensors of at most 256K elements (layer4 at the per-rank batch 32 of config 3)
static bool bn_cg_on(const Net& n, int64_t M, int C, bool dual) {
  return option_get(OPT_BN_CG) != 0 && !n.sync && !n.f32 && bn_fused() && M * C <= (int64_t)option_get(OPT_BN_CG_ELEMS) &&
         bn_bwd_cg_ok(M, C, dual);
}

// dx1 = BN-backward apply of b1 on (dz, x1) [; dx2 of b2 on (dz, x2)], coefficients from the sums
// a reduction accumulated; dgamma / dbeta into the flat gradient buffer. bf16 (T = u16) honours option
// bn_fused_fin and, with mask bits, forms dz = dy * bit itself (dzo: also stores it); fp32 always fuses.
template <typename T>
static int bn_bwd_coef_apply(Net& n, BNL& b1, const T* dz, const Nd<T>* x1, Nd<T>* dx1, BNL* b2, const Nd<T>* x2,
                             Nd<T>* dx2, int64_t M, float gs, hipStream_t st, const uint8_t* mbits = nullptr,
                             Nd<T>* dzo = nullptr) {
  constexpr bool bf = std::is_same<T, u16>::value;
  if (n.sync) {  // SyncBN backward: global sum(dz), sum(dz*xhat); dgamma/dbeta stay this rank's share
    DTC_TRY(sync_bn_sums(n, b1.acc, b1.C, st));
    if (b2) DTC_TRY(sync_bn_sums(n, b2->acc, b2->C, st));
    gs /= (float)n.sync_world;
  }
  const int64_t cnt = n.sync ? M * n.sync_world : M;
  if (!bf || bn_fused()) {
    const BnBwdArgs a1 = bwd_args(n, b1, cnt, gs);
    const BnBwdArgs a2 = b2 ? bwd_args(n, *b2, cnt, gs) : BnBwdArgs{};
    if constexpr (bf) {
      if (mbits) {
        PROF(3, (double)M * b1.C * (6.125 + (x2 ? 4.0 : 0.0) + (dzo ? 2.0 : 0.0)),
             bn_bwd_fin_apply_mask(dz, mbits, dzo, x1, a1, dx1, x2, b2 ? &a2 : nullptr, dx2, M, b1.C, st, ts));
        return 0;
      }
    }
    return bn_bwd_fin_apply(dz, x1, a1, dx1, x2, b2 ? &a2 : nullptr, dx2, M, b1.C, st);
  }
  if constexpr (bf) {
    DTC_CHECK_ARG(mbits == nullptr, "mask-bit BN backward needs the fused finalize");
    DTC_TRY(bn_bwd_finalize(n.at<int64_t>(b1.acc), b1.C, cnt, n.pf(b1.gidx), n.at<float>(b1.mean), n.at<float>(b1.invstd),
                            gs, n.gf(b1.gidx), n.gf(b1.bidx), n.at<float>(b1.coef), st));
    if (b2)
      DTC_TRY(bn_bwd_finalize(n.at<int64_t>(b2->acc), b2->C, cnt, n.pf(b2->gidx), n.at<float>(b2->mean),
                              n.at<float>(b2->invstd), gs, n.gf(b2->gidx), n.gf(b2->bidx), n.at<float>(b2->coef), st));
    return bn_bwd_apply(dz, x1, n.at<float>(b1.coef), dx1, x2, b2 ? n.at<float>(b2->coef) : nullptr, dx2, M, b1.C, st);
  }
  return 0;
}
// The mask-bit BN backward of the BN(s) of bundle r (dx1 [, dx2]; dzo: dz = dy * bit stored too, may alias dy):
// one launch for small tensors, else the reduction pass and the apply
static int bn_bwd_mask(Net& n, const BnbArgs& r, BNL& b1, const u16* dy, u16* dzo, u16* dx1, BNL* b2, u16* dx2,
                       int64_t M, float gs, hipStream_t st) {
  if (bn_cg_on(n, M, b1.C, b2 != nullptr)) {
    const BnBwdArgs a1 = bwd_args(n, b1, M, gs);
    const BnBwdArgs a2 = b2 ? bwd_args(n, *b2, M, gs) : BnBwdArgs{};
    PROF(3, (double)M * b1.C * (6.125 + (r.x2 ? 4.0 : 0.0) + (dzo ? 2.0 : 0.0)),
         bn_bwd_cg(dy, r.mb, dzo, r.x1, a1, dx1, r.x2, b2 ? &a2 : nullptr, dx2, M, b1.C, st, ts));
    return 0;
  }
  DTC_TRY(bn_reduce_mask(n, r, dy, M, b1.C, st));
  return bn_bwd_coef_apply(n, b1, dy, r.x1, dx1, b2, r.x2, dx2, M, gs, st, r.mb, dzo);
}

// The frame of every backward body. Prologue: profiling / marker cursors, the six gradient buffers as T, and
// the head (pool + Linear backward, the loss backward inside it with option xent_fuse) into G[0]; the BN
// backward sums were zeroed by the training forward. Epilogue: the last bucket point and the profile fold.
template <typename T>
static int bwd_begin(Net& n, const float* dlogits, float gs, const T* wfc, T* (&G)[6], hipStream_t st) {
  const Plan& p = n.plan;
  n.prof.next = ProfState::BWD0;
  n.side.ev_next = 0;
  for (int i = 0; i < 6; ++i) G[i] = n.at<T>(p.G[i]);
  const BlockL& last = n.blocks.back();
  return head_bwd(dlogits, n.at<float>(p.FEAT), wfc, n.B, last.Hout * last.Wout, 512, n.ncls, gs, n.gf(n.fc_w),
                  n.gf(n.fc_b), G[0], n.at<float>(p.HEADWS), p.HEADWS_bytes, st, n.xent.logits ? &n.xent : nullptr);
}
static int bwd_end(Net& n, const BwdCtx& cx, hipStream_t st) {
  DTC_TRY(maybe_bucket(n, -1, cx, st));
  if (n.prof.on) DTC_TRY(prof_accumulate(n.prof.ts, ProfState::SLOTS, n.prof.acc, st));
  return 0;
}
// the stem weight gradient from a stored conv-output gradient dc0 (bf16 bodies)
static int stem_wgrad_dc0(Net& n, const u16* dc0, float gs, hipStream_t st) {
  const Plan& p = n.plan;
  const int64_t M0 = (int64_t)n.B * n.H * n.W;
  float* slab = n.at<float>(p.SLAB);
  PROF(2, 2.0 * M0 * 64 * 27,
       p.stem_direct ? stem_wgrad(n.at<float>(p.XIN), dc0, n.gf(n.stem.pidx), gs, n.B, n.H, n.W, slab, p.slab_bytes, st, ts)
                     : conv_wgrad(n.stem.s, n.at<u16>(p.X0), dc0, n.gf(n.stem.pidx), 27, 27, gs, slab, p.slab_bytes, st, ts));
  return 0;
}

// ------------------------------------------------------------------ backward bodies
static int backward_body_f32(Net& n, const float* dlogits, float gs, const BwdCtx& cx, hipStream_t st) {
  const Plan& p = n.plan;
  float* G[6];
  DTC_TRY(bwd_begin(n, dlogits, gs, n.pf(n.fc_w), G, st));
  for (int bi = (int)n.blocks.size() - 1; bi >= 0; --bi) {
    BlockL& b = n.blocks[bi];
    const int64_t M = (int64_t)n.B * b.Hout * b.Wout;
    const float* in = bi > 0 ? n.at<float>(n.blocks[bi - 1].OUT) : n.at<float>(p.A0);
    float* dc2 = n.at<float>(b.DC2);
    float* dc1 = n.at<float>(b.DC1);
    float* dsc = b.proj ? n.at<float>(b.DSC) : nullptr;
    BNL* bsc = b.proj ? &b.bsc : nullptr;
    const float* s = b.proj ? n.at<float>(b.S) : nullptr;
    const std::string cp = cap_prefix(n, bi);
    DTC_TRY(cap(n, cp + ".dy", G[0], st));
    // out = relu(bn2(c2) + shortcut): dz = dy * [out > 0] and the BN-backward sums of bn2 (+ bn_sc)
    float* dz2 = G[1];
    DTC_TRY(bn_reduce(bnb_of_f32(n, b.OUT, b.C2, b.b2, b.S, bsc), G[0], dz2, M, b.Cout, st));
    DTC_TRY(bn_bwd_coef_apply(n, b.b2, dz2, n.at<float>(b.C2), dc2, bsc, s, dsc, M, gs, st));
    DTC_TRY(cap(n, cp + ".dz", dz2, st));
    DTC_TRY(cap(n, cp + ".dc2", dc2, st));
    if (b.proj) DTC_TRY(cap(n, cp + ".ds", dsc, st));
    DTC_TRY(f32_wgrad(n, b.c2.s, n.at<float>(b.A1), dc2, n.gf(b.c2.pidx), gs, st));
    DTC_TRY(f32_dgrad(n, b.c2.s, dc2, n.pf(b.c2.pidx), G[4], nullptr, st));
    DTC_TRY(cap(n, cp + ".da1", G[4], st));
    // a1 = relu(bn1(c1)): dz1 = da1 * [a1 > 0] (in place) and bn1's sums
    DTC_TRY(bn_reduce(bnb_of_f32(n, b.A1, b.C1, b.b1), G[4], G[4], M, b.Cout, st));
    DTC_TRY(cap(n, cp + ".dz1", G[4], st));
    DTC_TRY(bn_bwd_coef_apply(n, b.b1, G[4], n.at<float>(b.C1), dc1, nullptr, nullptr, nullptr, M, gs, st));
    DTC_TRY(cap(n, cp + ".dc1", dc1, st));
    DTC_TRY(f32_wgrad(n, b.c1.s, in, dc1, n.gf(b.c1.pidx), gs, st));
    if (b.proj) {
      DTC_TRY(f32_wgrad(n, b.sc.s, in, dsc, n.gf(b.sc.pidx), gs, st));
      DTC_TRY(f32_dgrad(n, b.sc.s, dsc, n.pf(b.sc.pidx), G[5], nullptr, st));
      DTC_TRY(cap(n, cp + ".dxs", G[5], st));
      DTC_TRY(f32_dgrad(n, b.c1.s, dc1, n.pf(b.c1.pidx), G[0], G[5], st));
    } else {  // dx = dgrad + dz2 (the identity shortcut's gradient)
      DTC_TRY(f32_dgrad(n, b.c1.s, dc1, n.pf(b.c1.pidx), G[0], dz2, st));
    }
    DTC_TRY(cap(n, cp + ".dx", G[0], st));
    DTC_TRY(maybe_bucket(n, bi, cx, st));
  }
  const int64_t M0 = (int64_t)n.B * n.H * n.W;
  float* dc0 = n.at<float>(p.DC0);
  DTC_TRY(bn_reduce(bnb_of_f32(n, p.A0, p.C0, n.bn0), G[0], G[1], M0, 64, st));
  DTC_TRY(bn_bwd_coef_apply(n, n.bn0, G[1], n.at<float>(p.C0), dc0, nullptr, nullptr, nullptr, M0, gs, st));
  DTC_TRY(cap(n, "grad.stem.dz", G[1], st));
  DTC_TRY(cap(n, "grad.stem.dc", dc0, st));
  DTC_TRY(f32_wgrad(n, f32_stem_shape(n), n.at<float>(p.X0), dc0, n.gf(n.stem.pidx), gs, st, 27, 2.0 * M0 * 64 * 27));
  return bwd_end(n, cx, st);
}

// Backward with the mask-bit BN path (bn_mask_on): G[0] carries the RAW gradient of a block output
// (never masked in place by a reduction), each BN reduction reads (dy, mask bits, x) and stores
// nothing, and each BN apply forms dz = dy * bit again. The identity shortcut needs dz itself (the
// residual of conv1's dgrad): bn2's apply writes it over dy in place (same lane reads then writes).
// (Every BN's backward sums come from a reduction pass of its own -- or the one-launch small-tensor kernel;
// the round-3/4 option that accumulated them in the producing dgrad's epilogue measured slower and was
// removed in round 5: DESIGN.md.)
static int backward_body_mask(Net& n, const float* dlogits, float gs, const BwdCtx& cx, hipStream_t st) {
  const Plan& p = n.plan;
  u16* G[6];
  DTC_TRY(bwd_begin(n, dlogits, gs, n.wbf(n.fc_w), G, st));
  float* slab = n.at<float>(p.SLAB);
  float* slabw = n.at<float>(p.SLABW);
  hipStream_t sd = st;  // weight-gradient stream
  const bool lazy = option_get(OPT_FORK_LAZY) != 0;
  WgQueue wq;
  for (int bi = (int)n.blocks.size() - 1; bi >= 0; --bi) {
    BlockL& b = n.blocks[bi];
    const int64_t M = (int64_t)n.B * b.Hout * b.Wout;
    const u16* in = bi > 0 ? n.at<u16>(n.blocks[bi - 1].OUT) : n.at<u16>(p.A0);
    u16* dc2 = n.at<u16>(b.DC2);
    u16* dc1 = n.at<u16>(b.DC1);
    u16* dsc = b.proj ? n.at<u16>(b.DSC) : nullptr;
    BNL* bsc = b.proj ? &b.bsc : nullptr;
    const BnbArgs r2 = bnb_out(n, b, true), r1 = bnb_of(n, b.MA1, b.C1, b.b1, 0, nullptr, true);
    const std::string cp = cap_prefix(n, bi);
    DTC_TRY(cap(n, cp + ".dy", G[0], st));
    DTC_TRY(cap_masked(n, cp + ".dz", G[0], b.MOUT, M, b.Cout, st));
    // out = relu(bn2(c2) + shortcut): sums of dz = dy * [out > 0] (and of the projection BN), then
    // dc2 (and dsc); an identity block also needs dz itself as conv1's dgrad residual: in place in G[0]
    DTC_TRY(bn_bwd_mask(n, r2, b.b2, G[0], b.proj ? nullptr : G[0], dc2, bsc, dsc, M, gs, st));
    DTC_TRY(cap(n, cp + ".dc2", dc2, st));
    if (b.proj) DTC_TRY(cap(n, cp + ".ds", dsc, st));
    // the shortcut's dx at its stride-2 grid only (option sc_compact): the 1x1 stride-2 conv's dgrad
    // is zero at three of four parities; conv1's parity-class dgrad adds it at the fourth
    const ConvRequest with_res{/*res=*/true};
    const ConvRoute dg1 = b.proj && !n.capture ? conv_route(b.c1.s, CONV_DGRAD, with_res) : ConvRoute{};
    const bool sc_cmp = option_get(OPT_SC_COMPACT) != 0 && dg1.kernel == CONV_K_GEMM_CLASSES;
    const ConvShape sc_dg = sc_cmp ? ConvShape{b.sc.s.N, b.Hout, b.Wout, b.sc.s.C, b.sc.s.K, 1, 1, 1, 0} : b.sc.s;
    // option dgrad_scf: the shortcut's dgrad as extra reduction steps of conv1's class-(0, 0) dgrad (one launch)
    const bool dscf = dg1.sc_ok;
    if (!lazy) DTC_TRY(fork_side(n, st, &sd));
    DTC_TRY(wg_issue(n, wq, b.c2.s, n.at<u16>(b.A1), dc2, n.gf(b.c2.pidx), gs, slabw, sd, st, lazy));
    PROF(1, conv_flops(b.c2.s),
         conv_dgrad(b.c2.s, dc2, n.wbf(b.c2.pidx), G[4], nullptr, slab, p.slab_bytes, st, ts, 0, n.tick(0)));
    DTC_TRY(cap(n, cp + ".da1", G[4], st));
    DTC_TRY(cap_masked(n, cp + ".dz1", G[4], b.MA1, M, b.Cout, st));
    DTC_TRY(bn_bwd_mask(n, r1, b.b1, G[4], nullptr, dc1, nullptr, nullptr, M, gs, st));
    DTC_TRY(cap(n, cp + ".dc1", dc1, st));
    if (!lazy || b.proj) DTC_TRY(fork_side(n, st, &sd));  // (the shortcut's wgrad below launches)
    // option wgrad_s2: conv1 (3x3 stride 2) and the shortcut (1x1 stride 2) weight gradients in one
    // column-split halo launch (x read once; the shortcut is conv1's centre tap against dsc)
    ConvRequest on_hand;
    on_hand.slab_bytes = p.slab_bytes;
    const ConvRoute wg1 = b.proj ? conv_route(b.c1.s, CONV_WGRAD, on_hand) : ConvRoute{};
    const bool wsc = wg1.sc_ok && b.sc.s.R == 1 && b.sc.s.stride == 2 && b.sc.s.C == b.c1.s.C && b.sc.s.K == b.c1.s.K;
    if (wsc) {
      PROF(2, conv_flops(b.c1.s) + conv_flops(b.sc.s),
           conv_wgrad_s2(b.c1.s, wg1.splits, in, dc1, dsc, n.gf(b.c1.pidx), n.gf(b.sc.pidx), gs, slabw, p.slab_bytes, sd,
                         ts));
    } else {
      DTC_TRY(wg_issue(n, wq, b.c1.s, in, dc1, n.gf(b.c1.pidx), gs, slabw, sd, st, lazy && !b.proj));
    }
    if (b.proj) {
      if (!wsc)
        PROF(2, conv_flops(b.sc.s),
             conv_wgrad(b.sc.s, in, dsc, n.gf(b.sc.pidx), 0, 0, gs, slabw, p.slab_bytes, sd, ts));
      if (dscf) {
        PROF(1, conv_flops(b.c1.s) + conv_flops(b.sc.s),
             conv_dgrad_sc(b.c1.s, dc1, n.wbf(b.c1.pidx), G[0], dsc, n.wbf(b.sc.pidx), st, ts));
      } else {
        PROF(1, conv_flops(b.sc.s),
             conv_dgrad(sc_dg, dsc, n.wbf(b.sc.pidx), G[5], nullptr, slab, p.slab_bytes, st, ts, 0, n.tick(0)));
        PROF(1, conv_flops(b.c1.s),
             conv_dgrad(b.c1.s, dc1, n.wbf(b.c1.pidx), G[0], G[5], slab, p.slab_bytes, st, ts, sc_cmp ? 1 : 0, n.tick(0)));
      }
      DTC_TRY(cap(n, cp + ".dxs", G[5], st));
    } else {  // residual = dz of this block's output (G[0], written by bn2's apply); dx over it in place
      PROF(1, conv_flops(b.c1.s),
           conv_dgrad(b.c1.s, dc1, n.wbf(b.c1.pidx), G[0], G[0], slab, p.slab_bytes, st, ts, 0, n.tick(0)));
    }
    DTC_TRY(cap(n, cp + ".dx", G[0], st));
    if (bucket_fires(n, bi)) DTC_TRY(wg_flush_forked(n, wq, gs, slabw, sd, st));
    DTC_TRY(maybe_bucket(n, bi, cx, st));
  }
  // stem: a0 = relu(bn1(conv1(x)))
  const int64_t M0 = (int64_t)n.B * n.H * n.W;
  u16* dc0 = n.at<u16>(p.DC0);
  const BnbArgs r0 = bnb_of(n, p.MA0, p.C0, n.bn0, 0, nullptr, true);
  // option stem_bn_fuse: the stem BN's apply runs inside the stem weight gradient (dc0 never stored;
  // not with parity captures, which want dc0, or SyncBN, whose sums are all-reduced first)
  const bool fused = p.stem_direct && !n.capture && !n.sync && bn_fused() && option_get(OPT_STEM_BN_FUSE) != 0;
  const bool ctj = n.ct.cur && !cx.capturing;  // a timed eager backward
  DTC_TRY(bn_reduce_mask(n, r0, G[0], M0, 64, st));
  if (!fused) {
    DTC_TRY(bn_bwd_coef_apply(n, n.bn0, G[0], r0.x1, dc0, nullptr, nullptr, nullptr, M0, gs, st, r0.mb));
    DTC_TRY(cap_masked(n, "grad.stem.dz", G[0], p.MA0, M0, 64, st));
    DTC_TRY(cap(n, "grad.stem.dc", dc0, st));
  }
  DTC_TRY(wg_flush_forked(n, wq, gs, slabw, sd, st));
  if (fused) {  // before the join: the kernel depends on nothing the side stream computes
    const BnBwdArgs a0 = bwd_args(n, n.bn0, M0, gs);
    PROF(2, 2.0 * M0 * 64 * 27,
         stem_wgrad_bn(n.at<float>(p.XIN), G[0], r0.mb, r0.x1, a0, n.gf(n.stem.pidx), gs, n.B, n.H, n.W, slab,
                       p.slab_bytes, st, ts));
  }
  if (ctj) DTC_HIP(hipEventRecord(n.ct.cur->join_c, st));
  DTC_TRY(join_side(n, st));
  if (ctj) {
    DTC_HIP(hipEventRecord(n.ct.cur->join_d, st));
    n.ct.cur->join = true;
  }
  // after the join: the stem wgrad is the last kernel, run on the main stream
  if (!fused) DTC_TRY(stem_wgrad_dc0(n, dc0, gs, st));
  if (ctj) {  // the last backward kernel of either stream has been issued: the tail starts here
    DTC_HIP(hipEventRecord(n.ct.cur->tail_a, st));
    n.ct.cur->tail = true;
  }
  return bwd_end(n, cx, st);
}

// bf16 without mask bits: the BN reductions read the post-ReLU outputs, right behind the producing dgrad
static int backward_body(Net& n, const float* dlogits, float gs, const BwdCtx& cx, hipStream_t st) {
  if (n.f32) return backward_body_f32(n, dlogits, gs, cx, st);
  if (bn_mask_on(n)) return backward_body_mask(n, dlogits, gs, cx, st);
  const Plan& p = n.plan;
  u16* G[6];
  DTC_TRY(bwd_begin(n, dlogits, gs, n.wbf(n.fc_w), G, st));
  float* slab = n.at<float>(p.SLAB);
  float* slabw = n.at<float>(p.SLABW);
  hipStream_t sd = st;  // weight-gradient stream
  // fuse: the dgrad producing a BN output's gradient is followed at once by that BN's backward reduction, in
  // place on dx (captures keep the unfused order: they record dy and dz separately)
  const bool fuse = !n.capture;
  bool dz_ready = false;  // G[0] already holds the next BN's dz (reduced in place behind the previous dgrad)
  WgQueue wq;
  for (int bi = (int)n.blocks.size() - 1; bi >= 0; --bi) {
    BlockL& b = n.blocks[bi];
    const int64_t M = (int64_t)n.B * b.Hout * b.Wout;
    const u16* in = bi > 0 ? n.at<u16>(n.blocks[bi - 1].OUT) : n.at<u16>(p.A0);
    u16* dc2 = n.at<u16>(b.DC2);
    u16* dc1 = n.at<u16>(b.DC1);
    u16* dsc = b.proj ? n.at<u16>(b.DSC) : nullptr;
    const std::string cp = cap_prefix(n, bi);
    DTC_TRY(cap(n, cp + ".dy", G[0], st));
    // out = relu(bn2(c2) + shortcut): dz = dy * [out > 0]
    u16* dz2 = G[0];
    if (!dz_ready) {
      dz2 = G[1];
      DTC_TRY(bn_reduce(bnb_out(n, b), G[0], dz2, M, b.Cout, st));
    }
    DTC_TRY(bn_bwd_coef_apply(n, b.b2, dz2, n.at<u16>(b.C2), dc2, b.proj ? &b.bsc : nullptr,
                              b.proj ? n.at<u16>(b.S) : nullptr, dsc, M, gs, st));
    DTC_TRY(cap(n, cp + ".dz", dz2, st));
    DTC_TRY(cap(n, cp + ".dc2", dc2, st));
    if (b.proj) DTC_TRY(cap(n, cp + ".ds", dsc, st));
    // conv2: dW2 (side stream) and da1
    DTC_TRY(fork_side(n, st, &sd));
    DTC_TRY(wg_issue(n, wq, b.c2.s, n.at<u16>(b.A1), dc2, n.gf(b.c2.pidx), gs, slabw, sd));
    // a1 = relu(bn1(c1)): da1 -> dz1 in place
    PROF(1, conv_flops(b.c2.s), conv_dgrad(b.c2.s, dc2, n.wbf(b.c2.pidx), G[4], nullptr, slab, p.slab_bytes, st, ts));
    if (!fuse) DTC_TRY(cap(n, cp + ".da1", G[4], st));
    DTC_TRY(bn_reduce(bnb_of(n, b.A1, b.C1, b.b1), G[4], G[4], M, b.Cout, st));
    DTC_TRY(cap(n, cp + ".dz1", G[4], st));
    DTC_TRY(bn_bwd_coef_apply(n, b.b1, G[4], n.at<u16>(b.C1), dc1, nullptr, nullptr, nullptr, M, gs, st));
    DTC_TRY(cap(n, cp + ".dc1", dc1, st));
    // conv1 (+ shortcut): weight grads (side stream), then the block-input gradient with the residual fused
    DTC_TRY(fork_side(n, st, &sd));
    DTC_TRY(wg_issue(n, wq, b.c1.s, in, dc1, n.gf(b.c1.pidx), gs, slabw, sd));
    if (b.proj) {
      PROF(2, conv_flops(b.sc.s), conv_wgrad(b.sc.s, in, dsc, n.gf(b.sc.pidx), 0, 0, gs, slabw, p.slab_bytes, sd, ts));
      PROF(1, conv_flops(b.sc.s), conv_dgrad(b.sc.s, dsc, n.wbf(b.sc.pidx), G[5], nullptr, slab, p.slab_bytes, st, ts));
      PROF(1, conv_flops(b.c1.s), conv_dgrad(b.c1.s, dc1, n.wbf(b.c1.pidx), G[0], G[5], slab, p.slab_bytes, st, ts));
    } else {  // fused: dz2 is G[0] and the dgrad updates it in place (residual read, dx written per element)
      PROF(1, conv_flops(b.c1.s), conv_dgrad(b.c1.s, dc1, n.wbf(b.c1.pidx), G[0], dz2, slab, p.slab_bytes, st, ts));
    }
    // the block input's gradient feeds the previous block's bn2 (+ its projection BN) or the stem BN
    if (fuse)
      DTC_TRY(bn_reduce(bi > 0 ? bnb_out(n, n.blocks[bi - 1]) : bnb_of(n, p.A0, p.C0, n.bn0), G[0], G[0],
                        (int64_t)b.c1.s.N * b.c1.s.H * b.c1.s.W, b.c1.s.C, st));
    dz_ready = fuse;
    if (b.proj) DTC_TRY(cap(n, cp + ".dxs", G[5], st));
    DTC_TRY(cap(n, cp + ".dx", G[0], st));
    if (bucket_fires(n, bi)) DTC_TRY(wg_flush(n, wq, gs, slabw, sd));
    DTC_TRY(maybe_bucket(n, bi, cx, st));
  }
  // stem: a0 = relu(bn1(conv1(x)))
  const int64_t M0 = (int64_t)n.B * n.H * n.W;
  u16* dc0 = n.at<u16>(p.DC0);
  u16* dz0 = G[0];
  if (!dz_ready) {
    dz0 = G[1];
    DTC_TRY(bn_reduce(bnb_of(n, p.A0, p.C0, n.bn0), G[0], dz0, M0, 64, st));
  }
  DTC_TRY(bn_bwd_coef_apply(n, n.bn0, dz0, n.at<u16>(p.C0), dc0, nullptr, nullptr, nullptr, M0, gs, st));
  DTC_TRY(cap(n, "grad.stem.dz", dz0, st));
  DTC_TRY(cap(n, "grad.stem.dc", dc0, st));
  DTC_TRY(wg_flush(n, wq, gs, slabw, sd));
  DTC_TRY(join_side(n, st));  // the stem wgrad is the last kernel: run it on the main stream
  DTC_TRY(stem_wgrad_dc0(n, dc0, gs, st));
  return bwd_end(n, cx, st);
}

static int backward_impl(Net& n, const float* dlogits, float gs, Comm* comm, hipStream_t st) {
  const Plan& p = n.plan;
  // the fork watch names a stream of this call: it does not outlive the backward, on any exit
  struct WatchReset {
    ~WatchReset() { g_fork_watch = ForkWatch{}; }
  } watch_reset;
  n.prof.st = st;
  if (!n.sums_fresh) DTC_TRY(zero_bytes(n.mem.ws + p.acc_lo, p.stats_hi - p.acc_lo, st));
  n.sums_fresh = false;
  if (!graphs_on(n, true, comm != nullptr)) {
    BwdCtx cx;
    cx.comm = comm;
    DTC_TRY(backward_body(n, dlogits, gs, cx, st));
  } else {
    GraphState& g = n.graph;
    const int pi = n.prof.on ? 1 : 0;
    if (!g.bwd_segs[pi].empty() && (g.bwd_gs[pi] != gs || g.bwd_comm[pi] != (comm != nullptr))) drop_graphs(n);
    if (g.bwd_segs[pi].empty()) {
      std::vector<Seg> segs;
      BwdCtx cx;
      cx.comm = comm;
      cx.capturing = true;
      cx.segs = &segs;
      Seg tail;
      int rc = begin_capture(n);
      if (rc == 0) rc = end_capture(n, backward_body(n, n.at<float>(p.DLOGITS), gs, cx, g.cap_st), &tail.exec);
      if (rc != 0) {
        for (auto& sg : segs)
          if (sg.exec) (void)hipGraphExecDestroy(sg.exec);
        return rc;
      }
      segs.push_back(tail);
      g.bwd_segs[pi] = segs;
      g.bwd_gs[pi] = gs;
      g.bwd_comm[pi] = comm != nullptr;
    }
    if (dlogits != n.at<float>(p.DLOGITS))
      DTC_HIP(hipMemcpyAsync(n.at<float>(p.DLOGITS), dlogits, (size_t)n.B * n.ncls * 4, hipMemcpyDeviceToDevice, st));
    // option comm_on_side: each bucket's collective on the weight-gradient stream forked from the compute
    // stream after its segment (that stream is idle between the replayed segments), joined once at the end:
    // no stream of the communicator's own in the backward
    const bool on_side = option_get(OPT_COMM_ON_SIDE) != 0 && comm != nullptr;
    for (const auto& sg : g.bwd_segs[pi]) {
      if (sg.exec) DTC_TRY(graph_launch(n, sg.exec, st));
      for (int i : sg.buckets) {
        hipStream_t sd = st;
        if (on_side) DTC_TRY(fork_side(n, st, &sd));
        DTC_TRY(issue_bucket(n, comm, i, sd, on_side));
      }
    }
    if (on_side) DTC_TRY(join_side(n, st));
  }
  if (comm) DTC_TRY(comm_join(comm, st));
  return 0;
}
static int backward(Net& n, const float* dlogits, float gs, Comm* comm, hipStream_t st) {
  n.ct.cur = nullptr;
  if (comm && n.ct.left > 0 && n.ct.used < (int)n.ct.steps.size()) {
    n.ct.cur = &n.ct.steps[n.ct.used++];
    --n.ct.left;
    n.ct.cur->join = n.ct.cur->tail = n.ct.cur->ok = false;
    n.ct.cur->bucket.assign(n.ct.cur->b0.size(), false);
    DTC_HIP(hipEventRecord(n.ct.cur->bwd0, st));
  }
  const int rc = backward_impl(n, dlogits, gs, comm, st);
  if (rc == 0 && n.ct.cur) {
    DTC_HIP(hipEventRecord(n.ct.cur->tail_b, st));  // after the Reducer's join
    n.ct.cur->ok = true;
  }
  n.ct.cur = nullptr;
  return rc;
}

// The loss backward and the backward in one call. Option xent_fuse: the eager backward's head kernel computes
// dlogits itself from `xa` (and still stores it into the dlogits buffer); a graph-replayed backward keeps the
// separate launch `unfused(dlogits)` (its head reads the buffer)
template <typename Unfused>
static int xent_backward(Net& n, const XentArgs& xa, Unfused unfused, float gs, Comm* comm, hipStream_t st) {
  float* dl = n.at<float>(n.plan.DLOGITS);
  if (option_get(OPT_XENT_FUSE) != 0 && !n.capture && !graphs_on(n, true, comm != nullptr)) {
    n.xent = xa;
    const int rc = backward(n, dl, gs, comm, st);
    n.xent = XentArgs();
    return rc;
  }
  DTC_TRY(unfused(dl));
  return backward(n, dl, gs, comm, st);
}

// STORE / ADD accumulate locally and reduce nothing (DDP's no_sync): a communicator there is a caller's mistake,
// refused before any launch
static int accum_args_ok(const char* fn, const Net& n, const void* comm) {
  DTC_CHECK_ARG(!(comm && (n.accum_mode == DTC_ACCUM_STORE || n.accum_mode == DTC_ACCUM_ADD)),
                "%s: gradient accumulation mode %d (STORE / ADD) takes no communicator: pass comm = NULL and "
                "all-reduce in the finishing backward", fn, n.accum_mode);
  return 0;
}

// the checks the two eval_batch entry points share, reported under the caller's name
static int eval_args_ok(const char* fn, const dtc_net* net, const float* x, const int64_t* labels, int n_valid,
                        int topk, const dtc_eval_record* rec) {
  DTC_CHECK_ARG(n_valid >= 1 && n_valid <= net->n.B && n_valid <= 4096,
                "%s: n_valid = %d outside [1, min(batch = %d, 4096)]", fn, n_valid, net->n.B);
  DTC_CHECK_ARG(topk >= 1 && topk <= net->n.ncls, "%s: topk = %d outside [1, num_classes = %d]", fn, topk,
                net->n.ncls);
  DTC_CHECK_ARG(net->n.mem.ws && x && labels && rec, "%s: unbound net or null pointer", fn);
  return 0;
}

}  // namespace dtc

// ------------------------------------------------------------------ C ABI (the run)
using namespace dtc;

extern "C" {

int dtc_rn18_forward(dtc_net* net, const float* x, float* logits, int train, void* stream) {
  DTC_CHECK_ARG(net && net->n.mem.ws && x && logits, "dtc_rn18_forward: unbound net or null pointer");
  DTC_TRY(forward(net->n, x, logits, train != 0, (hipStream_t)stream));
  if (train) net->n.sums_fresh = true;  // this forward zeroed the BN backward sums
  return 0;
}

int dtc_rn18_eval_batch(dtc_net* net, const float* x, const int64_t* labels, int n_valid, int topk, float* logits,
                        dtc_eval_record* rec, void* stream) {
  DTC_CHECK_ARG(net != nullptr, "dtc_rn18_eval_batch: null net");
  DTC_TRY(eval_args_ok("dtc_rn18_eval_batch", net, x, labels, n_valid, topk, rec));
  return eval_batch(net->n, x, labels, n_valid, topk, logits, rec, (hipStream_t)stream);
}

// The executor reads parameters, bf16 shadow and running statistics only through mem.p / mem.pb / mem.bufs (pf(),
// wbf(), the BN tables), and nothing derived from them outlives a forward: the stem's packed weight (WSTEM) is
// re-packed by every forward body, the BN coefficients are recomputed by every eval_batch. So evaluating other
// weights is the same eager eval_batch with the three pointers swapped for its duration. Captured graphs hold the
// bound pointers and are not touched (eval_batch replays none).
int dtc_rn18_eval_batch_weights(dtc_net* net, const float* params, const uint16_t* params_bf16, const float* bufs,
                                const float* x, const int64_t* labels, int n_valid, int topk, float* logits,
                                dtc_eval_record* rec, void* stream) {
  DTC_CHECK_ARG(net != nullptr, "dtc_rn18_eval_batch_weights: null net");
  DTC_CHECK_ARG(params && params_bf16 && bufs, "dtc_rn18_eval_batch_weights: null weight pointer");
  DTC_CHECK_ARG(((uintptr_t)params & 15) == 0 && ((uintptr_t)params_bf16 & 15) == 0,
                "dtc_rn18_eval_batch_weights: parameter buffers must be 16-byte aligned");
  DTC_TRY(eval_args_ok("dtc_rn18_eval_batch_weights", net, x, labels, n_valid, topk, rec));
  Bound& m = net->n.mem;
  const Bound bound = m;
  m.p = const_cast<float*>(params);  // the eval-mode forward only reads all three
  m.pb = const_cast<u16*>(params_bf16);
  m.bufs = const_cast<float*>(bufs);
  const int rc = eval_batch(net->n, x, labels, n_valid, topk, logits, rec, (hipStream_t)stream);
  m = bound;
  return rc;
}

int dtc_rn18_backward(dtc_net* net, const float* dlogits, float grad_scale, dtc_comm* comm, void* stream) {
  DTC_CHECK_ARG(net && net->n.mem.ws && dlogits, "dtc_rn18_backward: unbound net or null pointer");
  DTC_TRY(accum_args_ok("dtc_rn18_backward", net->n, comm));
  return backward(net->n, dlogits, grad_scale, (Comm*)comm, (hipStream_t)stream);
}

int dtc_rn18_xent_backward(dtc_net* net, const float* logits, const int64_t* labels, const float* lse,
                           const float* gscale, float grad_scale, dtc_comm* comm, void* stream) {
  DTC_CHECK_ARG(net && net->n.mem.ws && logits && labels && lse, "dtc_rn18_xent_backward: unbound net or null pointer");
  DTC_TRY(accum_args_ok("dtc_rn18_xent_backward", net->n, comm));
  Net& n = net->n;
  hipStream_t st = (hipStream_t)stream;
  const XentArgs xa{logits, labels, lse, gscale};
  auto unfused = [&](float* dl) { return xent_bwd(logits, labels, lse, gscale, n.B, n.ncls, dl, st); };
  return xent_backward(n, xa, unfused, grad_scale, (Comm*)comm, st);
}

int dtc_rn18_xent_soft_backward(dtc_net* net, const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                                const float* lam, float smoothing, const float* lse, const float* gscale,
                                float grad_scale, dtc_comm* comm, void* stream) {
  DTC_CHECK_ARG(net && net->n.mem.ws && logits && labels_a && lse,
                "dtc_rn18_xent_soft_backward: unbound net or null pointer");
  DTC_CHECK_ARG((labels_b != nullptr) == (lam != nullptr) && smoothing >= 0.f && smoothing <= 1.f,
                "dtc_rn18_xent_soft_backward: labels_b and lam go together, smoothing = %g must be in [0, 1]",
                (double)smoothing);
  DTC_TRY(accum_args_ok("dtc_rn18_xent_soft_backward", net->n, comm));
  Net& n = net->n;
  hipStream_t st = (hipStream_t)stream;
  const XentArgs xa{logits, labels_a, lse, gscale, labels_b ? labels_b : labels_a, lam, smoothing, true};
  auto unfused = [&](float* dl) {
    return xent_soft_bwd(logits, labels_a, labels_b, lam, smoothing, lse, gscale, n.B, n.ncls, dl, st);
  };
  return xent_backward(n, xa, unfused, grad_scale, (Comm*)comm, st);
}

}  // extern "C"
