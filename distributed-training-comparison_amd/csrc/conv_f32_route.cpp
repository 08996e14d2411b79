// Which kernel an fp32 convolution pass runs on and the slab that route wants: the one planner the fp32 executor
// (net_plan.cpp, net_run.cpp) and the dtc_conv2d_f32_* entry points (capi.cpp) ask. Every split-bf16 kernel keeps its
// feasibility predicate and its workspace function beside the kernel; only this file knows which predicate a pass
// answers to and at which level of option f32_split the executor asks for it (DESIGN.md section 7r has the table):
//
//   pass           launch                 level   predicate                 split kernel          slab of the split route
//   FWD / DGRAD    one conv                 1     conv_f32x_ok              conv_f32x             none
//   WGRAD          one conv                 2     conv_f32x_wgrad_ok        conv_f32x_wgrad       conv_f32x_wgrad_workspace
//   FWD / DGRAD    conv1 + shortcut pair    3     conv_f32x_s2_ok           conv_f32x_s2          none
//   WGRAD          conv1 + shortcut pair    4     conv_f32x_s2_wgrad_ok     conv_f32x_s2_wgrad    conv_f32x_s2_wgrad_workspace
//
// Everything else runs conv_f32 (the pair: two launches) on f32_conv_workspace's slab (the pair: the larger of the
// two, each launch takes the whole of it). FWD / DGRAD read the weights as bf16 planes, so they also need the planes;
// the weight gradients split all their operands themselves. Options are read at call time; nothing is cached.
#include "kernels.h"

namespace dtc {

// the level of option f32_split from which the executor asks for the split kernel: [pair][weight gradient]
static constexpr int SPLIT_LEVEL[2][2] = {{1, 2}, {3, 4}};

bool conv_f32_split_on(int pass, bool sc) { return option_get(OPT_F32_SPLIT) >= SPLIT_LEVEL[sc][pass == CONV_WGRAD]; }

ConvShape conv_f32_sc_shape(const ConvShape& s) { return ConvShape{s.N, s.H, s.W, s.C, s.K, 1, 1, s.stride, 0}; }

ConvF32Plan conv_f32_plan(const ConvShape& s, int pass, bool sc, bool want_split, bool planes) {
  const bool wgrad = pass == CONV_WGRAD;
  bool split = want_split && (wgrad || ((pass == CONV_FWD || pass == CONV_DGRAD) && planes));
  if (split) {
    if (sc) split = wgrad ? conv_f32x_s2_wgrad_ok(s) : conv_f32x_s2_ok(s, pass);
    else split = wgrad ? conv_f32x_wgrad_ok(s) : conv_f32x_ok(s);
  }
  ConvF32Plan r;
  if (split) {
    r.kernel = CONV_F32_SPLIT;
    r.slab_bytes = !wgrad ? 0 : sc ? conv_f32x_s2_wgrad_workspace(s) : conv_f32x_wgrad_workspace(s);
  } else {
    r.slab_bytes = f32_conv_workspace(s, pass);
    if (sc) r.slab_bytes = std::max(r.slab_bytes, f32_conv_workspace(conv_f32_sc_shape(s), pass));
  }
  return r;
}

}  // namespace dtc
