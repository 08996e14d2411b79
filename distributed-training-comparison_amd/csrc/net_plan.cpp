// ResNet-18 executor, planning: the layers and their flat parameter layout, the workspace plan (activation
// and capture registries, slab sizing), the DDP buckets, and the entry points that create, bind and query an
// executor. Nothing here launches a kernel.
#include <algorithm>
#include "flat.h"
#include "net.h"

namespace dtc {

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------ construction
static int add_param(Net& n, const std::string& name, std::vector<int64_t> shape, bool conv_krsc) {
  ParamEntry e;
  e.name = name;
  e.ndim = (int)shape.size();
  e.numel = 1;
  for (int i = 0; i < e.ndim; ++i) {
    e.shape[i] = shape[i];
    e.numel *= shape[i];
  }
  if (conv_krsc) {  // logical [K][C][R][S] stored as K R S C
    const int64_t C = shape[1], R = shape[2], S = shape[3];
    e.stride[0] = R * S * C;
    e.stride[1] = 1;
    e.stride[2] = S * C;
    e.stride[3] = C;
  } else {
    int64_t s = 1;
    for (int i = e.ndim - 1; i >= 0; --i) {
      e.stride[i] = s;
      s *= shape[i];
    }
  }
  n.params.push_back(e);
  return (int)n.params.size() - 1;
}

static void make_conv(Net& n, ConvL& c, const std::string& name, int N, int H, int W, int Cin, int Cout, int k,
                      int stride) {
  c.s = ConvShape{N, H, W, Cin, Cout, k, k, stride, k == 3 ? 1 : 0};
  c.P = (H + 2 * c.s.pad - k) / stride + 1;
  c.Q = (W + 2 * c.s.pad - k) / stride + 1;
  c.pidx = add_param(n, name, {Cout, Cin, k, k}, true);
}

static void make_bn(Net& n, BNL& b, const std::string& prefix, int C) {
  b.prefix = prefix;
  b.C = C;
  b.gidx = add_param(n, prefix + ".weight", {C}, false);
  b.bidx = add_param(n, prefix + ".bias", {C}, false);
}

static int build(Net& n) {
  const int B = n.B;
  // stem: registered as conv1.weight [64,3,3,3], bn1.{weight,bias}   (net.py:91-92)
  n.stem.s = ConvShape{B, n.H, n.W, 64, 64, 1, 1, 1, 0};  // GEMM over the 64-column im2col image
  n.stem.P = n.H;
  n.stem.Q = n.W;
  n.stem.pidx = add_param(n, "conv1.weight", {64, 3, 3, 3}, true);
  make_bn(n, n.bn0, "bn1", 64);
  // layers (net.py:93-96, _make_layer net.py:99-105)
  int in_planes = 64, H = n.H, W = n.W;
  const int planes[4] = {64, 128, 256, 512};
  const int strides[4] = {1, 2, 2, 2};
  for (int L = 0; L < 4; ++L) {
    for (int bi = 0; bi < 2; ++bi) {
      const int stride = bi == 0 ? strides[L] : 1;
      BlockL blk;
      const std::string pre = block_name(2 * L + bi);
      blk.Cin = in_planes;
      blk.Cout = planes[L];
      blk.Hin = H;
      blk.Win = W;
      make_conv(n, blk.c1, pre + ".conv1.weight", B, H, W, in_planes, planes[L], 3, stride);
      make_bn(n, blk.b1, pre + ".bn1", planes[L]);
      blk.Hout = blk.c1.P;
      blk.Wout = blk.c1.Q;
      make_conv(n, blk.c2, pre + ".conv2.weight", B, blk.Hout, blk.Wout, planes[L], planes[L], 3, 1);
      make_bn(n, blk.b2, pre + ".bn2", planes[L]);
      blk.proj = (stride != 1 || in_planes != planes[L]);  // net.py:28
      if (blk.proj) {
        make_conv(n, blk.sc, pre + ".shortcut.0.weight", B, H, W, in_planes, planes[L], 1, stride);
        make_bn(n, blk.bsc, pre + ".shortcut.1", planes[L]);
      }
      n.blocks.push_back(blk);
      in_planes = planes[L];
      H = blk.Hout;
      W = blk.Wout;
    }
  }
  n.fc_w = add_param(n, "linear.weight", {n.ncls, 512}, false);  // net.py:97
  n.fc_b = add_param(n, "linear.bias", {n.ncls}, false);
  if (H < 1 || W < 1) return set_error(DTC_EINVAL, "rn18: input %dx%d too small", n.H, n.W);

  // flat layout: reverse registration order, 64-element alignment
  int64_t off = 0;
  for (int i = (int)n.params.size() - 1; i >= 0; --i) {
    n.params[i].offset = off;
    off = align_up(off + n.params[i].numel, 64);
  }
  n.flat_numel = off;

  // BN registry in registration order and buffer layout
  n.bns.push_back(&n.bn0);
  for (auto& b : n.blocks) {
    n.bns.push_back(&b.b1);
    n.bns.push_back(&b.b2);
    if (b.proj) n.bns.push_back(&b.bsc);
  }
  int64_t boff = 0;
  for (size_t i = 0; i < n.bns.size(); ++i) {
    BNL* b = n.bns[i];
    b->rm_off = boff;
    boff = align_up(boff + b->C, 64);
    b->rv_off = boff;
    boff = align_up(boff + b->C, 64);
    b->nbt = (int)i;
  }
  n.bufs_numel = boff;
  for (auto& b : n.blocks)  // conv1.weight is the block's first-registered, hence highest, param
    b.grad_hi = align_up(n.params[b.c1.pidx].offset + n.params[b.c1.pidx].numel, 64);
  return 0;
}

static void plan_workspace(Net& n, float bucket_cap_mb) {
  Plan& p = n.plan;
  p.acts.clear();
  p.caps.clear();
  p.bucket_off.clear();
  p.bucket_len.clear();
  p.bucket_after_block.clear();
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off = (size_t)align_up((int64_t)(off + bytes), 256);
    return o;
  };
  const int64_t B = n.B;
  const int64_t M0 = B * n.H * n.W;
  const size_t E = n.esz();
  p.stem_direct = !n.f32 && option_get(OPT_STEM_DIRECT) != 0;
  p.XIN = p.stem_direct ? take(M0 * 3 * 4) : 0;
  p.X0 = p.stem_direct ? 0 : take(M0 * 64 * 2);  // im2col: [M0][64] bf16 or [M0][32] fp32
  p.WSTEM = take(64 * 64 * 2);
  p.C0 = take(M0 * 64 * E);
  p.A0 = take(M0 * 64 * E);
  p.MA0 = take(M0 * 64 / 8);
  int64_t gmax = M0 * 64;
  for (auto& b : n.blocks) {
    const int64_t M = B * b.Hout * b.Wout;
    const size_t bytes = M * b.Cout * E;
    b.C1 = take(bytes);
    b.A1 = take(bytes);
    b.C2 = take(bytes);
    if (b.proj) b.S = take(bytes);
    b.OUT = take(bytes);
    b.MA1 = take(M * b.Cout / 8);
    b.MOUT = take(M * b.Cout / 8);
    gmax = std::max<int64_t>(gmax, std::max<int64_t>(M * b.Cout, B * b.Hin * b.Win * b.Cin));
  }
  if (!p.stem_direct) p.acts.push_back({"stem.im2col", p.X0, (int)B, n.H, n.W, 64});
  p.acts.push_back({"stem.conv", p.C0, (int)B, n.H, n.W, 64});
  p.acts.push_back({"stem.out", p.A0, (int)B, n.H, n.W, 64});
  for (size_t i = 0; i < n.blocks.size(); ++i) {
    const BlockL& b = n.blocks[i];
    const std::string pre = block_name((int)i);
    p.acts.push_back({pre + ".conv1", b.C1, (int)B, b.Hout, b.Wout, b.Cout});
    p.acts.push_back({pre + ".relu1", b.A1, (int)B, b.Hout, b.Wout, b.Cout});
    p.acts.push_back({pre + ".conv2", b.C2, (int)B, b.Hout, b.Wout, b.Cout});
    if (b.proj) p.acts.push_back({pre + ".shortcut", b.S, (int)B, b.Hout, b.Wout, b.Cout});
    p.acts.push_back({pre + ".out", b.OUT, (int)B, b.Hout, b.Wout, b.Cout});
  }
  p.FEAT = take(B * 512 * 4);
  p.LOGITS = take(B * n.ncls * 4);
  p.DLOGITS = take(B * n.ncls * 4);
  p.HEADWS_bytes = head_bwd_workspace((int)B, 512, n.ncls);
  p.HEADWS = take(p.HEADWS_bytes);
  p.acts.push_back({"head.feat_f32", p.FEAT, (int)B, 1, 1, 512});
  for (int i = 0; i < 6; ++i) p.G[i] = take(gmax * E);
  for (auto& b : n.blocks) {  // per-block, so a pending side-stream wgrad never sees them overwritten
    const size_t bytes = (size_t)B * b.Hout * b.Wout * b.Cout * E;
    b.DC2 = take(bytes);
    b.DC1 = take(bytes);
    if (b.proj) b.DSC = take(bytes);
  }
  p.DC0 = take(M0 * 64 * E);
  p.PROF_TS = take((size_t)ProfState::SLOTS * DTC_PROF_SLOT_U64 * sizeof(u64));
  p.PROF_ACC = take((size_t)ProfState::SLOTS * 2 * sizeof(u64));
  // BN per-layer state
  p.stats_lo = off;  // forward statistics of every BN, then backward sums: both zeroed by the training forward
  for (BNL* b : n.bns) b->stats = take(DTC_STAT_WORDS(b->C) * 8);
  p.acc_lo = off;
  for (BNL* b : n.bns) b->acc = take(DTC_STAT_WORDS(b->C) * 8);
  p.BNERR = take(256);
  p.stats_hi = off;
  for (BNL* b : n.bns) {
    b->mean = take(b->C * 4);
    b->invstd = take(b->C * 4);
    b->scale = take(b->C * 4);
    b->shift = take(b->C * 4);
    b->coef = take(3 * b->C * 4);
  }
  // split-K slabs: max over every conv pass
  size_t slab = (size_t)64 * 64 * 4;
  auto consider = [&](const ConvShape& s) {
    for (int m = 0; m < 3; ++m)
      slab = std::max(slab, n.f32 ? f32_conv_workspace(s, m) : conv_route(s, m).slab_bytes);
  };
  auto consider_batch = [&](const ConvShape& s) {  // a bucket's 3x3 stride-1 wgrads, 2..DTC_WG_BATCH per launch
    ConvRequest rq;
    for (rq.nprob = 2; rq.nprob <= DTC_WG_BATCH; ++rq.nprob)
      if (const ConvRoute r = conv_route(s, CONV_WGRAD, rq); r.kernel == CONV_K_WGRAD_HALO)
        slab = std::max(slab, r.slab_bytes);
  };
  consider(n.f32 ? f32_stem_shape(n) : n.stem.s);
  for (auto& b : n.blocks) {
    consider(b.c1.s);
    consider(b.c2.s);
    if (b.proj) consider(b.sc.s);
    if (!n.f32) {  // (conv1 + shortcut in one wgrad_s2 launch: its slab is conv1's own WGRAD route's)
      consider_batch(b.c1.s);
      consider_batch(b.c2.s);
    }
  }
  if (p.stem_direct) slab = std::max(slab, stem_wgrad_slab_bytes(M0));
  p.slab_bytes = slab;
  p.SLAB = take(slab);
  p.SLABW = take(slab);
  p.TICK = take((size_t)DTC_TICKS * 4);  // zeroed at bind; every in-kernel split-K leaves its counters zero
  if (n.capture) {
    auto cap = [&](const std::string& nm, int h, int w, int c) {
      p.caps.push_back({nm, take((size_t)B * h * w * c * E), (int)B, h, w, c});
    };
    for (size_t i = 0; i < n.blocks.size(); ++i) {
      const BlockL& b = n.blocks[i];
      const std::string pre = "grad." + block_name((int)i);
      for (const char* k : {".dy", ".dz", ".dc2", ".da1", ".dz1", ".dc1"}) cap(pre + k, b.Hout, b.Wout, b.Cout);
      if (b.proj) {
        cap(pre + ".ds", b.Hout, b.Wout, b.Cout);
        cap(pre + ".dxs", b.Hin, b.Win, b.Cin);
      }
      cap(pre + ".dx", b.Hin, b.Win, b.Cin);
    }
    cap("grad.stem.dz", n.H, n.W, 64);
    cap("grad.stem.dc", n.H, n.W, 64);
  }
  p.ws_bytes = off;

  // gradient buckets at block granularity in backward order (head + layer4.1 first); a bucket
  // closes once it holds >= bucket_cap_mb (torch DDP's rule). Option bucket_tail (default 1; a
  // deviation from torch's cap semantics, reported in the bench line's buckets_mb): whatever is open
  // when layer2's backward ends also closes there if it is >= 1 MB, so the last bucket -- issued after
  // the stem, overlapping nothing -- is only layer1 + the stem (0.6 MB, the unavoidable tail of SURVEY
  // A.2) instead of up to the whole cap
  const int64_t cap = (int64_t)(bucket_cap_mb * 1024.0 * 1024.0 / 4.0);
  const bool tail_split = option_get(OPT_BUCKET_TAIL) != 0;
  int64_t start = 0;
  for (int bi = (int)n.blocks.size() - 1; bi >= 0 && cap > 0; --bi) {
    const int64_t hi = n.blocks[bi].grad_hi;
    const bool tail_edge = tail_split && bi == 2 && n.blocks.size() == 8;  // layer2.0: next come layer1 and the stem
    if (hi - start >= cap || (tail_edge && (hi - start) * 4 >= (1 << 20))) {
      p.bucket_off.push_back(start);
      p.bucket_len.push_back(hi - start);
      p.bucket_after_block.push_back(bi);
      start = hi;
    }
  }
  p.bucket_off.push_back(start);
  p.bucket_len.push_back(n.flat_numel - start);
  p.bucket_after_block.push_back(-1);
}

// one entry of the activation / capture registry
static int act_info(const char* fn, const std::vector<Act>* table, int idx, const char** name, size_t* ws_offset,
                    int* shape4) {
  DTC_CHECK_ARG(table && idx >= 0 && idx < (int)table->size(), "%s: bad index", fn);
  const Act& a = (*table)[idx];
  if (name) *name = a.name.c_str();
  if (ws_offset) *ws_offset = a.off;
  if (shape4) {
    shape4[0] = a.n; shape4[1] = a.h; shape4[2] = a.w; shape4[3] = a.c;
  }
  return 0;
}

}  // namespace dtc

// ------------------------------------------------------------------ C ABI (planning and queries)
using namespace dtc;

extern "C" {

int dtc_rn18_create(dtc_net** out, int batch, int height, int width, int num_classes, float bucket_cap_mb) {
  DTC_CHECK_ARG(out != nullptr, "dtc_rn18_create: null out");
  DTC_CHECK_ARG(batch > 0 && height >= 8 && width >= 8 && num_classes > 0, "dtc_rn18_create: bad shape");
  // Kernels whose buffer descriptors take 32-bit byte offsets (conv_c64, conv_halo, wgrad_halo, the
  // igemm fast wgrad loader) gate themselves on tensors < 2 GiB and the executor falls back to the
  // 64-bit-addressed implicit-GEMM loaders above that (224x224 at batch > 333). What remains is the
  // element index of the largest activation, [batch, height, width, 64]: it must fit an int32
  // (224x224: batch <= 684; BASELINE config 5 is 512).
  DTC_CHECK_ARG((int64_t)batch * height * width * 64 < (1ll << 31),
                "dtc_rn18_create: activation too large (batch*height*width*64 elements >= 2^31)");
  dtc_net* h = new dtc_net();
  h->n.B = batch;
  h->n.H = height;
  h->n.W = width;
  h->n.ncls = num_classes;
  int r = build(h->n);
  if (r) {
    delete h;
    return r;
  }
  h->bucket_cap_mb = bucket_cap_mb;
  plan_workspace(h->n, bucket_cap_mb);
  *out = h;
  return 0;
}

int dtc_rn18_destroy(dtc_net* net) {
  if (net) {
    Net& n = net->n;
    drop_graphs(n);
    ct_free(n);
    if (n.graph.cap_st) (void)hipStreamDestroy(n.graph.cap_st);
    if (n.side.st) (void)hipStreamDestroy(n.side.st);
    for (auto& e : n.side.evs)
      if (e) (void)hipEventDestroy(e);
    if (n.graph.launch_ev) (void)hipEventDestroy(n.graph.launch_ev);
  }
  delete net;
  return 0;
}

int dtc_rn18_num_params(const dtc_net* net) { return net ? (int)net->n.params.size() : DTC_EINVAL; }

int dtc_rn18_param_info(const dtc_net* net, int idx, const char** name, int64_t* offset, int64_t* numel, int* ndim,
                        int64_t* shape4, int64_t* stride4) {
  DTC_CHECK_ARG(net && idx >= 0 && idx < (int)net->n.params.size(), "dtc_rn18_param_info: bad index");
  const ParamEntry& e = net->n.params[idx];
  if (name) *name = e.name.c_str();
  if (offset) *offset = e.offset;
  if (numel) *numel = e.numel;
  if (ndim) *ndim = e.ndim;
  for (int i = 0; i < 4; ++i) {
    if (shape4) shape4[i] = e.shape[i];
    if (stride4) stride4[i] = e.stride[i];
  }
  return 0;
}

int64_t dtc_rn18_flat_numel(const dtc_net* net) { return net ? net->n.flat_numel : DTC_EINVAL; }
int dtc_rn18_num_bn(const dtc_net* net) { return net ? (int)net->n.bns.size() : DTC_EINVAL; }

int dtc_rn18_bn_info(const dtc_net* net, int idx, const char** prefix, int* channels, int64_t* mean_offset,
                     int64_t* var_offset) {
  DTC_CHECK_ARG(net && idx >= 0 && idx < (int)net->n.bns.size(), "dtc_rn18_bn_info: bad index");
  const BNL* b = net->n.bns[idx];
  if (prefix) *prefix = b->prefix.c_str();
  if (channels) *channels = b->C;
  if (mean_offset) *mean_offset = b->rm_off;
  if (var_offset) *var_offset = b->rv_off;
  return 0;
}

int64_t dtc_rn18_bufs_numel(const dtc_net* net) { return net ? net->n.bufs_numel : DTC_EINVAL; }
size_t dtc_rn18_workspace_bytes(const dtc_net* net) { return net ? net->n.plan.ws_bytes : 0; }
int dtc_rn18_num_buckets(const dtc_net* net) { return net ? (int)net->n.plan.bucket_off.size() : DTC_EINVAL; }

int dtc_rn18_bucket_info(const dtc_net* net, int idx, int64_t* offset, int64_t* numel) {
  DTC_CHECK_ARG(net && idx >= 0 && idx < (int)net->n.plan.bucket_off.size(), "dtc_rn18_bucket_info: bad index");
  if (offset) *offset = net->n.plan.bucket_off[idx];
  if (numel) *numel = net->n.plan.bucket_len[idx];
  return 0;
}

int dtc_rn18_bind(dtc_net* net, void* workspace, float* params, float* grads, uint16_t* params_bf16, float* bufs,
                  int64_t* num_batches_tracked, void* stream) {
  DTC_CHECK_ARG(net && workspace && params && grads && params_bf16 && bufs, "dtc_rn18_bind: null pointer");
  DTC_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "dtc_rn18_bind: workspace must be 256-byte aligned");
  DTC_CHECK_ARG(((uintptr_t)params_bf16 & 15) == 0 && ((uintptr_t)params & 15) == 0 && ((uintptr_t)grads & 15) == 0,
                "dtc_rn18_bind: parameter buffers must be 16-byte aligned");
  Net& n = net->n;
  n.mem.ws = (char*)workspace;
  n.mem.p = params;
  n.mem.g = grads;
  n.mem.pb = params_bf16;
  n.mem.bufs = bufs;
  n.mem.nbt = num_batches_tracked;
  n.accum_mode = DTC_ACCUM_OFF;  // the accumulation buffer was checked against the previous gradients
  n.accum = nullptr;
  n.compress_mode = DTC_COMPRESS_OFF;  // (likewise the staging buffer)
  n.compress = nullptr;
  n.prof.ts = n.at<u64>(n.plan.PROF_TS);
  n.prof.acc = n.at<u64>(n.plan.PROF_ACC);
  drop_graphs(n);  // captured launches hold the previous pointers
  DTC_HIP(hipMemsetAsync(n.mem.ws + n.plan.stats_lo, 0, n.plan.stats_hi - n.plan.stats_lo, (hipStream_t)stream));
  DTC_HIP(hipMemsetAsync(n.mem.ws + n.plan.TICK, 0, (size_t)DTC_TICKS * 4, (hipStream_t)stream));
  return 0;
}

int dtc_rn18_enable_capture(dtc_net* net) {
  DTC_CHECK_ARG(net && net->n.mem.ws == nullptr, "dtc_rn18_enable_capture: call before dtc_rn18_bind");
  net->n.capture = true;
  plan_workspace(net->n, net->bucket_cap_mb);
  return 0;
}

int dtc_rn18_set_precision(dtc_net* net, int fp32) {
  DTC_CHECK_ARG(net && net->n.mem.ws == nullptr, "dtc_rn18_set_precision: call before dtc_rn18_bind");
  net->n.f32 = fp32 != 0;
  plan_workspace(net->n, net->bucket_cap_mb);
  return 0;
}

int dtc_rn18_precision(const dtc_net* net) { return net ? (net->n.f32 ? 1 : 0) : DTC_EINVAL; }

int dtc_rn18_num_captures(const dtc_net* net) { return net ? (int)net->n.plan.caps.size() : DTC_EINVAL; }
int dtc_rn18_capture_info(const dtc_net* net, int idx, const char** name, size_t* ws_offset, int* shape4) {
  return act_info("dtc_rn18_capture_info", net ? &net->n.plan.caps : nullptr, idx, name, ws_offset, shape4);
}

int dtc_rn18_num_activations(const dtc_net* net) { return net ? (int)net->n.plan.acts.size() : DTC_EINVAL; }
int dtc_rn18_activation_info(const dtc_net* net, int idx, const char** name, size_t* ws_offset, int* shape4) {
  return act_info("dtc_rn18_activation_info", net ? &net->n.plan.acts : nullptr, idx, name, ws_offset, shape4);
}

int dtc_rn18_dlogits_buffer(const dtc_net* net, size_t* ws_offset) {
  DTC_CHECK_ARG(net && ws_offset, "dtc_rn18_dlogits_buffer: bad args");
  *ws_offset = net->n.plan.DLOGITS;
  return 0;
}

int dtc_rn18_set_grad_accum(dtc_net* net, float* acc, int mode) {
  DTC_CHECK_ARG(net != nullptr, "dtc_rn18_set_grad_accum: null net");
  DTC_CHECK_ARG(mode >= DTC_ACCUM_OFF && mode <= DTC_ACCUM_FINISH, "dtc_rn18_set_grad_accum: mode = %d outside [0, 3]",
                mode);
  Net& n = net->n;
  if (mode != DTC_ACCUM_OFF) {
    DTC_CHECK_ARG(acc != nullptr, "dtc_rn18_set_grad_accum: mode %d needs an accumulation buffer (acc is NULL)", mode);
    DTC_CHECK_ARG(n.mem.g != nullptr, "dtc_rn18_set_grad_accum: call after dtc_rn18_bind");
  }
  if (acc != nullptr) {
    DTC_CHECK_ARG(aligned(acc, 16), "dtc_rn18_set_grad_accum: acc must be 16-byte aligned");
    DTC_CHECK_ARG(n.mem.g == nullptr || !ranges_overlap(acc, n.flat_numel * 4, n.mem.g, n.flat_numel * 4),
                  "dtc_rn18_set_grad_accum: acc overlaps the bound gradient buffer");
  }
  n.accum = acc;
  n.accum_mode = mode;
  return 0;
}

int dtc_rn18_set_grad_compress(dtc_net* net, uint16_t* staging, int mode) {
  DTC_CHECK_ARG(net != nullptr, "dtc_rn18_set_grad_compress: null net");
  DTC_CHECK_ARG(mode == DTC_COMPRESS_OFF || mode == DTC_COMPRESS_BF16,
                "dtc_rn18_set_grad_compress: mode = %d is neither DTC_COMPRESS_OFF (0) nor DTC_COMPRESS_BF16 (1)", mode);
  Net& n = net->n;
  if (mode != DTC_COMPRESS_OFF) {
    DTC_CHECK_ARG(staging != nullptr, "dtc_rn18_set_grad_compress: mode %d needs a staging buffer (staging is NULL)",
                  mode);
    DTC_CHECK_ARG(n.mem.g != nullptr, "dtc_rn18_set_grad_compress: call after dtc_rn18_bind");
  }
  if (staging != nullptr) {
    DTC_CHECK_ARG(aligned(staging, 16), "dtc_rn18_set_grad_compress: staging must be 16-byte aligned");
    DTC_CHECK_ARG(n.mem.g == nullptr || !ranges_overlap(staging, n.flat_numel * 2, n.mem.g, n.flat_numel * 4),
                  "dtc_rn18_set_grad_compress: staging overlaps the bound gradient buffer");
  }
  n.compress = staging;
  n.compress_mode = mode;
  return 0;
}

int dtc_rn18_set_sync_bn(dtc_net* net, dtc_comm* comm) {
  DTC_CHECK_ARG(net != nullptr, "dtc_rn18_set_sync_bn: null net");
  Net& n = net->n;
  n.sync = (Comm*)comm;
  n.sync_world = comm ? comm_world((Comm*)comm) : 1;
  drop_graphs(n);
  return 0;
}

}  // extern "C"
