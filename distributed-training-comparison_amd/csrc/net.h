// ResNet-18 (CIFAR variant) training-step executor: the state shared by its three translation units.
//
//   net_plan.cpp  layers, flat parameter layout, workspace plan, DDP buckets; the planning / query entry points
//   net_run.cpp   graph capture, forward / evaluation / backward bodies and their entry points
//   net_prof.cpp  profiling slots, event brackets, communication timing and their entry points
//
// Mirrors the module structure of the reference (src/ddp/net.py:13-45 BasicBlock, net.py:86-116 ResNet,
// net.py:119-120 ResNet18).
//
// Parameter memory: one flat fp32 buffer in REVERSE registration order, 64-element aligned.
// Backward visits layers from the head to the stem, i.e. it finishes gradients in increasing
// address order, so every DDP bucket is a contiguous prefix-extension of the buffer.
#pragma once
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include "../../include/dtc.h"
#include "comm.h"
#include "kernels.h"

namespace dtc {

struct ParamEntry {
  std::string name;
  int64_t offset = 0, numel = 0;
  int ndim = 0;
  int64_t shape[4] = {0, 0, 0, 0};
  int64_t stride[4] = {0, 0, 0, 0};
};

struct ConvL {
  ConvShape s{};
  int P = 0, Q = 0;
  int pidx = -1;  // param index of the weight
};

struct BNL {
  std::string prefix;
  int C = 0;
  int gidx = -1, bidx = -1;  // param indices of weight (gamma) and bias (beta)
  int64_t rm_off = 0, rv_off = 0;
  int nbt = 0;
  size_t stats = 0, acc = 0, mean = 0, invstd = 0, scale = 0, shift = 0, coef = 0;  // workspace byte offsets
};

struct BlockL {
  ConvL c1, c2, sc;
  BNL b1, b2, bsc;
  bool proj = false;
  int Cin = 0, Cout = 0, Hin = 0, Win = 0, Hout = 0, Wout = 0;
  size_t C1 = 0, A1 = 0, C2 = 0, S = 0, OUT = 0;  // activation buffers (workspace byte offsets)
  size_t MA1 = 0, MOUT = 0;  // ReLU mask bits of A1 / OUT (bf16 executor, option bn_mask)
  size_t DC2 = 0, DC1 = 0, DSC = 0;  // backward: conv-output gradients read by the (side-stream) wgrads
  int64_t grad_hi = 0;  // end of this block's flat region: after its backward, [0, grad_hi) is complete
};

// activation / capture registry entry (per-layer parity): name, workspace byte offset, N,H,W,C
struct Act { std::string name; size_t off; int n, h, w, c; };

// Workspace byte offsets and buckets: written by plan_workspace only
struct Plan {
  size_t ws_bytes = 0;
  size_t X0 = 0, WSTEM = 0, C0 = 0, A0 = 0, FEAT = 0, G[6] = {0, 0, 0, 0, 0, 0}, SLAB = 0;
  size_t MA0 = 0;  // ReLU mask bits of A0
  size_t XIN = 0;  // executor-owned copy of the fp32 NCHW input (direct stem conv, bf16 mode)
  bool stem_direct = false;  // planned with option stem_direct (bf16): stem.hip instead of im2col + GEMM
  size_t HEADWS = 0, HEADWS_bytes = 0;
  size_t DC0 = 0, SLABW = 0;  // stem conv-output gradient; split-K slab of the side-stream wgrads
  size_t TICK = 0;            // split-K arrival counters of the compute stream's convs (the only in-kernel split-K)
  size_t BNERR = 0;           // int: set by a one-pass BN backward whose grid barrier timed out
  size_t slab_bytes = 0;
  size_t stats_lo = 0, acc_lo = 0, stats_hi = 0;  // BN slot regions [stats_lo, acc_lo), [acc_lo, stats_hi)
  // profiling slots: in the caller-owned workspace, so the slot pointers baked into the profiled graphs stay
  // valid for the executor's lifetime and arming / disarming profiling neither frees memory nor destroys
  // graphs (it switches between the two graph sets)
  size_t PROF_TS = 0, PROF_ACC = 0;
  size_t LOGITS = 0, DLOGITS = 0;  // graph-owned copies of the caller's logits / dlogits
  // buckets: [offset, numel) in flat elements, and the block index after whose backward it fires
  std::vector<int64_t> bucket_off, bucket_len;
  std::vector<int> bucket_after_block;  // -1 = after the stem (last)
  std::vector<Act> acts;  // activation registry
  std::vector<Act> caps;  // optional capture of backward intermediates (parity tests): name -> slot
};

// Memory bound by dtc_rn18_bind (eval_batch_weights swaps p / pb / bufs for one call)
struct Bound {
  char* ws = nullptr;  // workspace (Plan offsets)
  float *p = nullptr, *g = nullptr, *bufs = nullptr;  // flat parameters, flat gradients, BN running statistics
  u16* pb = nullptr;                                   // bf16 shadow of p
  int64_t* nbt = nullptr;                              // num_batches_tracked per BN (optional)
};

// hipGraph replay (option "graphs"): the forward per train flag, the backward as segments split
// at bucket boundaries (the all-reduces stay eager on the communicator's side stream)
struct Seg { hipGraphExec_t exec = nullptr; std::vector<int> buckets; };
struct GraphState {
  hipStream_t cap_st = nullptr;
  bool cap_locked = false;  // this executor holds g_graph_mu (between begin_capture and end_capture)
  int epoch = -1;
  // graph sets indexed [profiling]: the profiled set carries the timing stamps and the per-step fold
  hipGraphExec_t fwd_exec[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [profiling][train]
  std::vector<Seg> bwd_segs[2];
  float bwd_gs[2] = {0.f, 0.f};
  bool bwd_comm[2] = {false, false};
  // recorded on the launch stream after every graph launch: drop_graphs waits for it before destroying
  hipEvent_t launch_ev = nullptr;
  bool launched = false;
};

// backward weight gradients run on a side stream (option bwd_streams), overlapped with the
// data-gradient / BN chain; forked after the conv-output gradient exists, joined at bucket points
struct SideState {
  hipStream_t st = nullptr;
  bool pending = false;
  std::vector<hipEvent_t> evs;  // fork / join markers, used round robin
  int ev_next = 0;
};

struct ProfState {
  // live conv timing (bench roofline): each conv call stamps min(start)/max(end) of its workgroups
  // (s_memrealtime) into its own slot; one kernel per step folds the slots into running totals.
  // Graph-safe: the slot pointers are baked at capture, nothing happens on the host per call.
  static constexpr int SLOTS = 256, BWD0 = 96;  // forward calls use [0,96), backward [96,256)
  bool on = false;
  u64* ts = nullptr;   // [SLOTS][DTC_PROF_SLOT_U64] device (Plan::PROF_TS)
  u64* acc = nullptr;  // [SLOTS][2] device: (sum ticks, calls) (Plan::PROF_ACC)
  int next = 0;
  int kind[SLOTS] = {};
  double flops[SLOTS] = {};
  int khz = 100000;
  // event timing (dtc_rn18_profile_events; bench.py's roofline, the serialized eager step): every timed
  // launcher call is bracketed by two timing events on the compute stream -- its launch duration as a
  // rocprofv3 kernel trace of the same step sees it (dispatch to completion), summed per kind at the end
  bool events = false;
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> evpool;  // 2 per bracketed call, created up front
  size_t evn = 0;                  // pairs used
  long long evdropped = 0;         // calls that found the pool used up (not bracketed: reported)
  std::vector<std::pair<int, double>> evwork;  // (kind, work) per pair
};

// communication timing (dtc_rn18_comm_timing; bench.py's comm_exposed_us / buckets_us at N > 1): for the
// next `left` backward calls with a communicator, timing events on the streams the work runs on -- the
// backward's start (compute stream), each bucket collective's start / end (its own stream), the compute
// stream's wait for the weight-gradient stream before the stem weight gradient (join_c -> join_d), and the
// tail from the last backward kernel to the Reducer's join (tail_a -> tail_b)
struct CommTimes {
  hipEvent_t bwd0 = nullptr, join_c = nullptr, join_d = nullptr, tail_a = nullptr, tail_b = nullptr;
  std::vector<hipEvent_t> b0, b1;  // per bucket
  bool join = false, tail = false;  // join_c / join_d, tail_a recorded (eager backward)
  bool ok = false;                  // the backward succeeded and recorded tail_b (only these steps count)
  std::vector<bool> bucket;        // bucket i recorded
};
struct CommTiming {
  std::vector<CommTimes> steps;  // one per armed step
  int left = 0, used = 0;
  CommTimes* cur = nullptr;  // the set of the backward in progress (null: not timed)
};

struct Net {
  int B = 0, H = 0, W = 0, ncls = 100;
  // fp32 mode (dtc_rn18_set_precision): fp32 activations, f32-MFMA convs, fp32 BN / head -- the
  // reference without --amp (ddp/trainer.py:160-165). Default: bf16 activations (autocast).
  bool f32 = false;
  size_t esz() const { return f32 ? 4 : 2; }
  bool capture = false;  // parity captures planned (dtc_rn18_enable_capture)
  // SyncBatchNorm: per-channel BN sums all-reduced over this communicator
  // (its own, never the Reducer's, so the two collective streams cannot interleave on one comm)
  Comm* sync = nullptr;
  int sync_world = 1;
  // Gradient accumulation (dtc_rn18_set_grad_accum): the mode of the next backwards (DTC_ACCUM_*) and the
  // caller-owned buffer in the gradient buffer's layout; applied per bucket at the plan's bucket points
  int accum_mode = 0;
  float* accum = nullptr;
  // Gradient compression (dtc_rn18_set_grad_compress): the mode of the next backwards (DTC_COMPRESS_*) and the
  // caller-owned bf16 staging buffer in the gradient buffer's element layout; a backward with a communicator
  // all-reduces each bucket there and widens it back into the gradients behind the collective
  int compress_mode = 0;
  u16* compress = nullptr;
  // layers
  std::vector<ParamEntry> params;
  int64_t flat_numel = 0;
  int64_t bufs_numel = 0;
  ConvL stem;
  BNL bn0;
  std::vector<BlockL> blocks;
  std::vector<BNL*> bns;  // registration order
  int fc_w = -1, fc_b = -1;

  Plan plan;
  Bound mem;
  GraphState graph;
  SideState side;
  ProfState prof;
  CommTiming ct;

  // per-call state of the run
  // the backward sums [acc_lo, stats_hi) are zeroed by every training forward; a backward that finds
  // them already used (a second backward over one forward) zeroes them first instead of adding onto
  // the previous backward's sums
  bool sums_fresh = false;
  // set by eval_batch around its forward body: one bn_eval_coef_all launch already wrote every BN's scale /
  // shift (and mean / invstd), so the eval branch of bn_act skips the per-BN coefficient launches
  bool coef_ready = false;
  // dtc_rn18_xent_backward with option xent_fuse: the CrossEntropyLoss backward's inputs, consumed by the
  // head backward kernel (one launch fewer after the per-step barrier); set only for that call
  XentArgs xent;

  template <typename T>
  T* at(size_t off) const { return (T*)(mem.ws + off); }
  const u16* wbf(int pidx) const { return mem.pb + params[pidx].offset; }
  float* pf(int pidx) const { return mem.p + params[pidx].offset; }
  float* gf(int pidx) const { return mem.g + params[pidx].offset; }
  unsigned* tick(int i) { return (unsigned*)(mem.ws + plan.TICK) + (size_t)i * DTC_TICKS; }
};

// "layerL.B" of block i (registration names, activation / capture registry)
inline std::string block_name(int i) { return "layer" + std::to_string(i / 2 + 1) + "." + std::to_string(i % 2); }
// fp32 stem: a 1x1 "conv" over the 32-column fp32 im2col image (27 taps + 5 zero columns)
inline ConvShape f32_stem_shape(const Net& n) { return ConvShape{n.B, n.H, n.W, 32, 64, 1, 1, 1, 0}; }
inline double conv_flops(const ConvShape& s) {
  const int P = (s.H + 2 * s.pad - s.R) / s.stride + 1, Q = (s.W + 2 * s.pad - s.S) / s.stride + 1;
  return 2.0 * s.N * P * Q * (double)s.K * s.R * s.S * s.C;
}
// the weight gradients run on a side stream (option bwd_streams)
inline bool side_on() { return option_get(OPT_BWD_STREAMS) != 0; }

// net_run.cpp
extern std::recursive_mutex g_graph_mu;  // serialises graph capture, graph destruction and device drains
void drop_graphs(Net& n);

// net_prof.cpp
// kinds: 0 conv forward, 1 conv dgrad, 2 conv wgrad (work = algorithmic FLOPs), 3 BN family (work =
// algorithmic HBM bytes: the tensors each BN kernel must read / write once)
u64* prof_slot(Net& n, int kind, double flops);
// event bracket of one launcher call (-1: not recorded -- events off, a capture in progress, the weight
// gradients on a side stream the compute-stream events would not cover, or the pool used up)
int prof_ev_open(Net& n, int kind, double work);
void prof_ev_close(Net& n, int i);
void ct_free(Net& n);

// one timed launcher call: `call` sees its slot as `ts`
#define PROF(kind, flops, call)                        \
  do {                                                 \
    u64* ts = prof_slot(n, (kind), (flops));           \
    const int pev_ = prof_ev_open(n, (kind), (flops)); \
    const int prc_ = (call);                           \
    prof_ev_close(n, pev_);                            \
    DTC_TRY(prc_);                                     \
  } while (0)

}  // namespace dtc

struct dtc_net {
  dtc::Net n;
  float bucket_cap_mb = 25.f;
};
