// extern "C" entry points of libdtc_amd.so (declared in include/dtc.h) and the thread-local
// error channel. Each wrapper validates arguments, forwards to the C++ launcher and returns
// its status; no exception or exit() crosses this boundary.
#include <cstdarg>
#include <cstdio>
#include <string>
#include "../../include/dtc.h"
#include "comm.h"
#include "kernels.h"

#include <atomic>
#include <cstring>
#include <cstdlib>
#include <dlfcn.h>
#include <fcntl.h>
#include <execinfo.h>
#include <pthread.h>
#include <signal.h>
#include <sys/syscall.h>
#include <unistd.h>

namespace dtc {
static std::atomic<int> g_opts[OPT_COUNT] = {
#define DTC_OPT_DEF(id, name, def) {def},
    DTC_OPTION_LIST(DTC_OPT_DEF)
#undef DTC_OPT_DEF
};
static const char* g_opt_names[OPT_COUNT] = {
#define DTC_OPT_NAME(id, name, def) #name,
    DTC_OPTION_LIST(DTC_OPT_NAME)
#undef DTC_OPT_NAME
};
static std::atomic<int> g_epoch{0};
// DTC_OPTIONS="name=value,name=value" in the environment overrides defaults at library load (A/B and
// bisection runs of whole test suites without code changes)
static int apply_env_options() {
  const char* e = getenv("DTC_OPTIONS");
  if (!e) return 0;
  std::string s(e);
  size_t pos = 0;
  while (pos < s.size()) {
    size_t end = s.find(',', pos);
    if (end == std::string::npos) end = s.size();
    const std::string kv = s.substr(pos, end - pos);
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) {
      const std::string k = kv.substr(0, eq);
      const int v = atoi(kv.c_str() + eq + 1);
      for (int i = 0; i < OPT_COUNT; ++i)
        if (k == g_opt_names[i]) g_opts[i].store(v);
    }
    pos = end + 1;
  }
  return 1;
}
static const int g_env_applied = apply_env_options();
int option_get(int id) { return g_opts[id].load(std::memory_order_relaxed); }
int option_epoch() { return g_epoch.load(std::memory_order_relaxed); }
int option_set(const char* name, int value) {
  for (int i = 0; i < OPT_COUNT; ++i)
    if (name && strcmp(name, g_opt_names[i]) == 0) {
      g_opts[i].store(value, std::memory_order_relaxed);
      g_epoch.fetch_add(1, std::memory_order_relaxed);
      return 0;
    }
  return set_error(DTC_EINVAL, "unknown option %s", name ? name : "(null)");
}

static thread_local std::string g_err;
int set_error(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
const char* last_error() { return g_err.c_str(); }
}  // namespace dtc

using namespace dtc;

// ------------------------------------------------------------------ native crash report (diagnostics)
// dtc_install_crash_handler(): on SIGSEGV / SIGBUS / SIGFPE / SIGABRT print the faulting THREAD (tid,
// name) and its native frames (library + nearest exported symbol + offset) to stderr, then hand the
// signal to the previous handler (Python's faulthandler prints the Python threads). faulthandler alone
// cannot say in which native thread -- ours or a runtime worker -- a fault happened.
static struct sigaction g_prev_sa[32];
// the report also goes to the file DTC_CRASH_LOG names (opened at install): under pytest's fd capture, fd 2 of a
// test is a temporary file that is lost with the process (r06s: a SIGSEGV left only faulthandler's frames)
static int g_crash_fd = -1;
static void put(const char* s) {
  (void)!write(2, s, strlen(s));
  if (g_crash_fd >= 0) (void)!write(g_crash_fd, s, strlen(s));
}
static void put_hex(uintptr_t v) {
  char b[19] = "0x";
  for (int i = 0; i < 16; ++i) b[2 + i] = "0123456789abcdef"[(v >> (60 - 4 * i)) & 15];
  b[18] = 0;
  put(b);
}
static void crash_report(int sig, siginfo_t* si, void* uc) {
  char name[32] = {0};
  (void)pthread_getname_np(pthread_self(), name, sizeof(name));
  put("\n=== dtc crash report: signal ");
  put(sig == SIGSEGV ? "SIGSEGV" : sig == SIGBUS ? "SIGBUS" : sig == SIGFPE ? "SIGFPE" : "SIGABRT");
  put(" addr ");
  put_hex((uintptr_t)(si ? si->si_addr : nullptr));
  put(" tid ");
  put_hex((uintptr_t)syscall(SYS_gettid));
  put(" pid ");
  put_hex((uintptr_t)getpid());
  put(" thread '");
  put(name);
  put("'\n");
  void* fr[48];
  const int nf = backtrace(fr, 48);
  for (int i = 0; i < nf; ++i) {
    Dl_info d;
    put("  #");
    put_hex((uintptr_t)i);
    put(" ");
    if (dladdr(fr[i], &d) && d.dli_fname) {
      put(d.dli_fname);
      put(" +");
      put_hex((uintptr_t)fr[i] - (uintptr_t)d.dli_fbase);
      if (d.dli_sname) {
        put(" ");
        put(d.dli_sname);
        put(" +");
        put_hex((uintptr_t)fr[i] - (uintptr_t)d.dli_saddr);
      }
    } else {
      put_hex((uintptr_t)fr[i]);
    }
    put("\n");
  }
  put("=== end dtc crash report\n");
  // our own disposition goes first (a re-entry ends in the default action, never a loop), and
  // the previous handler is called only when it is not this one -- if Python's faulthandler was enabled
  // again after us, each records the other as "previous" and chaining both ways would recurse
  signal(sig, SIG_DFL);
  const struct sigaction& p = g_prev_sa[sig];
  if ((p.sa_flags & SA_SIGINFO) && p.sa_sigaction && p.sa_sigaction != crash_report) {
    p.sa_sigaction(sig, si, uc);
  } else if (!(p.sa_flags & SA_SIGINFO) && p.sa_handler != SIG_IGN && p.sa_handler != SIG_DFL && p.sa_handler) {
    p.sa_handler(sig);
  }
  signal(sig, SIG_DFL);
  raise(sig);
}

static inline hipStream_t S(void* s) { return (hipStream_t)s; }
static inline ConvShape shape_of(const dtc_conv_desc* d) {
  return ConvShape{d->n, d->h, d->w, d->c, d->k, d->r, d->s, d->stride, d->pad};
}
// The convolutions the kernels implement: 1x1 / 3x3, stride 1 / 2, pad 0 / 1, C and K multiples of 64,
// a non-empty output. Checked at the boundary, before any planning arithmetic (which divides by C / 64).
static bool desc_ok(const dtc_conv_desc* d) {
  if (!d || d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->k <= 0) return false;
  if (d->c % 64 != 0 || d->k % 64 != 0 || d->r != d->s || (d->r != 1 && d->r != 3)) return false;
  if ((d->stride != 1 && d->stride != 2) || d->pad < 0 || d->pad > 1) return false;
  const int64_t p = (d->h + 2 * d->pad - d->r) / d->stride + 1, q = (d->w + 2 * d->pad - d->s) / d->stride + 1;
  return p > 0 && q > 0 && (int64_t)d->n * d->h * d->w * std::max(d->c, d->k) < (1ll << 40);
}

#define GUARD(body)                                                          \
  try {                                                                      \
    body                                                                     \
  } catch (...) {                                                            \
    return set_error(DTC_EINVAL, "%s: unexpected C++ exception", __func__); \
  }

extern "C" {

int dtc_abi_version(void) { return DTC_ABI_VERSION; }
int dtc_set_option(const char* name, int value) { return option_set(name, value); }
int dtc_get_option(const char* name) {
  for (int i = 0; i < OPT_COUNT; ++i)
    if (name && strcmp(name, g_opt_names[i]) == 0) return option_get(i);
  return set_error(DTC_EINVAL, "unknown option %s", name ? name : "(null)");
}
const char* dtc_last_error(void) { return last_error(); }

int dtc_install_crash_handler(void) {
  static std::atomic<int> once{0};
  if (once.exchange(1)) return 0;
  void* warm[2];
  (void)backtrace(warm, 2);  // loads the unwinder now, not inside the handler
  if (const char* path = getenv("DTC_CRASH_LOG")) g_crash_fd = open(path, O_WRONLY | O_CREAT | O_APPEND, 0644);
  static char altstack[1 << 16];
  stack_t ss;
  ss.ss_sp = altstack;
  ss.ss_size = sizeof(altstack);
  ss.ss_flags = 0;
  (void)sigaltstack(&ss, nullptr);
  for (int sig : {SIGSEGV, SIGBUS, SIGFPE, SIGABRT}) {
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_sigaction = crash_report;
    sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
    sigemptyset(&sa.sa_mask);
    if (sigaction(sig, &sa, &g_prev_sa[sig]) != 0) return set_error(DTC_EINVAL, "sigaction failed");
  }
  return 0;
}

size_t dtc_conv2d_workspace_size(const dtc_conv_desc* d, int pass) {
  if (!desc_ok(d) || pass < 0 || pass > 2) return 0;
  const size_t slab = conv_route(shape_of(d), pass).slab_bytes;
  // FWD / DGRAD split-K: + the arrival counters of the in-kernel reduction at the workspace's end (+ room to
  // align them to 256 B, so a workspace of exactly this size always holds both)
  return slab > 0 && pass != 2 ? slab + (size_t)DTC_TICKS * 4 + 256 : slab;
}

// FWD / DGRAD workspace: [split-K slab][DTC_TICKS u32 arrival counters] when it holds both (the counters of
// the in-kernel reduction are zeroed on the call's stream first; the workspace is scratch between calls),
// else the whole of it is slab and a split-K plan reduces in a separate launch. Nothing is carved out (and
// nothing zeroed) when the plan has no slab or the in-kernel reduction is off (option splitk_ink). WGRAD: all of
// it is slab, except that dtc_conv2d_wgrad_sc's size query reserves DTC_TICKS words behind its slab and the entry
// point holds the caller to that layout. ws_carve is pure (the route query asks it too); op_ws adds the memset.
struct WsCarve {
  size_t slab_bytes;  // fp32 slab on hand (0 without a workspace)
  unsigned* tick;     // the arrival counters, or nullptr
};
static WsCarve ws_carve(const dtc_conv_desc* d, int pass, bool sc, const void* ws, size_t ws_bytes) {
  const size_t tb = (size_t)DTC_TICKS * 4;
  WsCarve c{ws ? ws_bytes : 0, nullptr};
  if (pass == CONV_WGRAD) {
    if (sc) c.slab_bytes = c.slab_bytes >= tb ? c.slab_bytes - tb : 0;
    return c;
  }
  const size_t slab = conv_route(shape_of(d), pass).slab_bytes;
  if (ws == nullptr || slab == 0 || ws_bytes < slab + tb || option_get(OPT_SPLITK_INK) == 0) return c;
  const uintptr_t end = ((uintptr_t)ws + ws_bytes - tb) & ~(uintptr_t)255;
  if (end < (uintptr_t)ws + slab) return c;
  return WsCarve{(size_t)(end - (uintptr_t)ws), (unsigned*)end};
}
static WsCarve op_ws(const dtc_conv_desc* d, int pass, void* ws, size_t ws_bytes, hipStream_t st) {
  const WsCarve c = ws_carve(d, pass, false, ws, ws_bytes);
  if (c.tick && hipMemsetAsync(c.tick, 0, (size_t)DTC_TICKS * 4, st) != hipSuccess) return WsCarve{ws ? ws_bytes : 0, nullptr};
  return c;
}

static_assert(DTC_CONV_K_GEMM == CONV_K_GEMM && DTC_CONV_K_GEMM_CLASSES == CONV_K_GEMM_CLASSES &&
                  DTC_CONV_K_C64 == CONV_K_C64 && DTC_CONV_K_HALO == CONV_K_HALO &&
                  DTC_CONV_K_DGRAD_S2 == CONV_K_DGRAD_S2 && DTC_CONV_K_WGRAD_HALO == CONV_K_WGRAD_HALO &&
                  DTC_CONV_K_WGRAD_S2 == CONV_K_WGRAD_S2,
              "DTC_CONV_K_* mirror ConvKernel");
static int route_answer(const ConvShape& s, int pass, const ConvRequest& rq, bool ticks, dtc_conv_route* out) {
  const ConvLaunch l = conv_launch(s, pass, rq);
  const ConvRoute& r = l.route;
  const bool gemm = r.kernel == CONV_K_GEMM || r.kernel == CONV_K_GEMM_CLASSES;
  const bool halo = r.kernel == CONV_K_HALO;
  memset(out, 0, sizeof(*out));
  out->kernel = r.kernel;
  out->gemm_bm = gemm ? r.gemm.bm : 0;
  out->gemm_bn = gemm ? r.gemm.bn : 0;
  out->splits = gemm ? r.gemm.splits : halo ? r.halo.split : r.splits > 0 ? r.splits : 1;
  out->halo_cfg = halo ? r.halo.cfg : -1;
  out->halo_gen = halo ? r.halo.gen : 0;
  out->reduce_in_kernel = ticks && halo && r.halo.split > 1;
  out->sc_ok = r.sc_ok;
  out->refused = l.refused != nullptr;
  out->slab_wanted = r.slab_bytes;
  out->slab_used = l.slab_used;
  return 0;
}

int dtc_conv2d_route_query(const dtc_conv_desc* d, int pass, int flags, int nprob, const void* ws, size_t ws_bytes,
                           dtc_conv_route* out) {
  DTC_CHECK_ARG(d && out, "dtc_conv2d_route_query: null argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_route_query: unsupported convolution descriptor");
  const bool res = (flags & DTC_CONV_ROUTE_RES) != 0, sc = (flags & DTC_CONV_ROUTE_SC) != 0;
  DTC_CHECK_ARG(pass >= 0 && pass <= 2 && nprob >= 1 && nprob <= DTC_WG_BATCH && (flags & ~3) == 0 &&
                    (!res || pass == CONV_DGRAD) && (nprob == 1 || (pass == CONV_WGRAD && !sc)) && !(res && sc),
                "dtc_conv2d_route_query: pass %d flags %d nprob %d name no entry point", pass, flags, nprob);
  const WsCarve c = ws_carve(d, pass, sc, ws, ws_bytes);
  ConvRequest rq;
  rq.res = res;
  rq.sc = sc;
  rq.nprob = nprob;
  rq.batch = nprob > 1;
  rq.slab_bytes = c.slab_bytes;
  GUARD(return route_answer(shape_of(d), pass, rq, c.tick != nullptr, out);)
}

int dtc_conv2d_fwd(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t* stats, void* ws,
                   size_t ws_bytes, void* stream) {
  DTC_CHECK_ARG(d && x && w && y, "dtc_conv2d_fwd: null argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_fwd: unsupported convolution descriptor");
  const WsCarve c = op_ws(d, CONV_FWD, ws, ws_bytes, S(stream));
  GUARD(return conv_fwd(shape_of(d), x, w, y, stats, (float*)ws, c.slab_bytes, S(stream), nullptr, c.tick);)
}

int dtc_conv2d_fwd_sc(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t* stats,
                      const uint16_t* wsc, uint16_t* ysc, int64_t* stats_sc, void* stream) {
  DTC_CHECK_ARG(d && x && w && y && wsc && ysc, "dtc_conv2d_fwd_sc: null argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_fwd_sc: unsupported convolution descriptor");
  const ConvShape s = shape_of(d);
  const ConvShape sc{s.N, s.H, s.W, s.C, s.K, 1, 1, 2, 0};
  GUARD(return conv_fwd_sc(s, sc, x, w, y, stats, wsc, ysc, stats_sc, S(stream));)
}

int dtc_conv2d_dgrad(const dtc_conv_desc* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx, const uint16_t* res,
                     void* ws, size_t ws_bytes, void* stream) {
  DTC_CHECK_ARG(d && dy && w && dx, "dtc_conv2d_dgrad: null argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_dgrad: unsupported convolution descriptor");
  const WsCarve c = op_ws(d, CONV_DGRAD, ws, ws_bytes, S(stream));
  GUARD(return conv_dgrad(shape_of(d), dy, w, dx, res, (float*)ws, c.slab_bytes, S(stream), nullptr, 0, c.tick);)
}

// the data gradient, then the BN-backward reduction of the post-ReLU BN output it is the gradient of, in place on dx
int dtc_conv2d_dgrad_bn(const dtc_conv_desc* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx,
                        const uint16_t* res, const uint16_t* ymask, const uint16_t* x1, const float* mean1,
                        const float* invstd1, int64_t* acc1, const uint16_t* x2, const float* mean2,
                        const float* invstd2, int64_t* acc2, void* ws, size_t ws_bytes, void* stream) {
  DTC_CHECK_ARG(d && dy && w && dx && ymask && x1 && mean1 && invstd1 && acc1, "dtc_conv2d_dgrad_bn: null argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_dgrad_bn: unsupported convolution descriptor");
  DTC_CHECK_ARG(!x2 || (mean2 && invstd2 && acc2), "dtc_conv2d_dgrad_bn: second BN arguments");
  const ConvShape s = shape_of(d);
  const WsCarve c = op_ws(d, CONV_DGRAD, ws, ws_bytes, S(stream));
  GUARD(DTC_TRY(conv_dgrad(s, dy, w, dx, res, (float*)ws, c.slab_bytes, S(stream), nullptr, 0, c.tick));
        return bn_bwd_reduce(dx, ymask, x1, mean1, invstd1, acc1, x2, mean2, invstd2, acc2, dx, (int64_t)s.N * s.H * s.W,
                             s.C, S(stream));)
}

int dtc_conv2d_dgrad_sc(const dtc_conv_desc* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx,
                        const uint16_t* dsc, const uint16_t* wsc, void* stream) {
  DTC_CHECK_ARG(d && dy && w && dx && dsc && wsc, "dtc_conv2d_dgrad_sc: null argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_dgrad_sc: unsupported convolution descriptor");
  GUARD(return conv_dgrad_sc(shape_of(d), dy, w, dx, dsc, wsc, S(stream));)
}

int dtc_conv2d_wgrad(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* dy, float* dw, float scale, void* ws,
                     size_t ws_bytes, void* stream) {
  DTC_CHECK_ARG(d && x && dy && dw && ws, "dtc_conv2d_wgrad: null argument (workspace is required)");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_wgrad: unsupported convolution descriptor");
  GUARD(return conv_wgrad(shape_of(d), x, dy, dw, 0, 0, scale, (float*)ws, ws_bytes, S(stream));)
}

size_t dtc_conv2d_wgrad_sc_workspace_size(const dtc_conv_desc* d) {
  if (!desc_ok(d)) return 0;
  const ConvRoute r = conv_route(shape_of(d), CONV_WGRAD);
  return r.sc_ok ? r.slab_bytes + (size_t)DTC_TICKS * 4 : 0;
}

int dtc_conv2d_wgrad_sc(const dtc_conv_desc* d, const uint16_t* x, const uint16_t* dy, const uint16_t* dsc, float* dw,
                        float* dw_sc, float scale, void* ws, size_t ws_bytes, void* stream) {
  DTC_CHECK_ARG(d && x && dy && dsc && dw && dw_sc, "dtc_conv2d_wgrad_sc: null argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_wgrad_sc: unsupported convolution descriptor");
  const WsCarve c = ws_carve(d, CONV_WGRAD, true, ws, ws_bytes);
  GUARD(return conv_wgrad_sc(shape_of(d), x, dy, dsc, dw, dw_sc, scale, (float*)ws, c.slab_bytes, S(stream));)
}

size_t dtc_conv2d_wgrad_batch_workspace_size(const dtc_conv_desc* d, int n) {
  if (!desc_ok(d) || n < 1 || n > DTC_WG_BATCH) return 0;
  ConvRequest rq;
  rq.nprob = n;
  const ConvRoute r = conv_route(shape_of(d), CONV_WGRAD, rq);
  return r.kernel == CONV_K_WGRAD_HALO ? r.slab_bytes : 0;
}

int dtc_conv2d_wgrad_batch(const dtc_conv_desc* d, int n, const uint16_t* const* x, const uint16_t* const* dy,
                           float* const* dw, float scale, void* ws, size_t ws_bytes, void* stream) {
  DTC_CHECK_ARG(d && x && dy && dw && ws && n >= 1 && n <= DTC_WG_BATCH, "dtc_conv2d_wgrad_batch: bad argument");
  DTC_CHECK_ARG(desc_ok(d), "dtc_conv2d_wgrad_batch: unsupported convolution descriptor");
  for (int i = 0; i < n; ++i) DTC_CHECK_ARG(x[i] && dy[i] && dw[i], "dtc_conv2d_wgrad_batch: null problem %d", i);
  GUARD(return conv_wgrad_batch(shape_of(d), n, x, dy, dw, scale, (float*)ws, ws_bytes, S(stream));)
}

size_t dtc_bn_stat_words(int c) { return c > 0 ? DTC_STAT_WORDS(c) : 0; }

int dtc_bn_stat_totals(const int64_t* w, int c, double* totals) {
  DTC_CHECK_ARG(w && totals && c > 0, "dtc_bn_stat_totals: bad args");
  for (int j = 0; j < 2; ++j)
    for (int ch = 0; ch < c; ++ch) {
      int64_t hi = 0, lo = 0;
      for (int k = 0; k < DTC_STAT_SLOTS; ++k) {
        hi += w[stat_word(k, j, 0, c) + ch];
        lo += w[stat_word(k, j, 1, c) + ch];
      }
      totals[(size_t)j * c + ch] = stat_total(hi, lo, w[0]);
    }
  return 0;
}

int dtc_bn_fwd_finalize(int64_t* stats, int c, int64_t count, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, int64_t* nbt, float momentum, float eps, float* mean,
                        float* invstd, float* scale, float* shift, void* stream) {
  return bn_fwd_finalize(stats, c, count, gamma, beta, running_mean, running_var, nbt, momentum, eps, mean, invstd,
                         scale, shift, S(stream));
}
int dtc_bn_apply_relu(const uint16_t* x, const float* scale, const float* shift, uint16_t* y, int64_t m, int c,
                      void* stream) {
  return bn_apply_relu(x, scale, shift, y, m, c, S(stream));
}
int dtc_bn_apply_add_relu(const uint16_t* x, const float* scale, const float* shift, const uint16_t* res, uint16_t* y,
                          int64_t m, int c, void* stream) {
  return bn_apply_add_relu(x, scale, shift, res, y, m, c, S(stream));
}
int dtc_bn_apply_dual_relu(const uint16_t* x, const float* scale, const float* shift, const uint16_t* x2,
                           const float* scale2, const float* shift2, uint16_t* y, int64_t m, int c, void* stream) {
  return bn_apply_dual_relu(x, scale, shift, x2, scale2, shift2, y, m, c, S(stream));
}
int dtc_bn_bwd_reduce(const uint16_t* dy, const uint16_t* ymask, const uint16_t* x1, const float* mean1,
                      const float* invstd1, int64_t* acc1, const uint16_t* x2, const float* mean2, const float* invstd2,
                      int64_t* acc2, uint16_t* dz, int64_t m, int c, void* stream) {
  return bn_bwd_reduce(dy, ymask, x1, mean1, invstd1, acc1, x2, mean2, invstd2, acc2, dz, m, c, S(stream));
}
int dtc_bn_bwd_finalize(int64_t* acc, int c, int64_t count, const float* gamma, const float* mean, const float* invstd,
                        float gscale, float* dgamma, float* dbeta, float* coef, void* stream) {
  return bn_bwd_finalize(acc, c, count, gamma, mean, invstd, gscale, dgamma, dbeta, coef, S(stream));
}
int dtc_bn_bwd_apply(const uint16_t* dz, const uint16_t* x1, const float* coef1, uint16_t* dx1, const uint16_t* x2,
                     const float* coef2, uint16_t* dx2, int64_t m, int c, void* stream) {
  return bn_bwd_apply(dz, x1, coef1, dx1, x2, coef2, dx2, m, c, S(stream));
}

int dtc_bn_fin_apply(int mode, const uint16_t* x, const int64_t* stats, int64_t count, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, int64_t* nbt, float momentum,
                     float eps, float* mean, float* invstd, const uint16_t* x2, const int64_t* stats2,
                     const float* gamma2, const float* beta2, float* running_mean2, float* running_var2,
                     int64_t* nbt2, float* mean2, float* invstd2, uint16_t* y, uint8_t* mask_bits, int64_t m, int c,
                     void* stream) {
  DTC_CHECK_ARG(mode >= 1 && mode <= 3, "dtc_bn_fin_apply: mode %d (1 relu, 2 add + relu, 3 dual + relu)", mode);
  DTC_CHECK_ARG(x && stats && gamma && beta && mean && invstd && y, "dtc_bn_fin_apply: null argument");
  DTC_CHECK_ARG(m > 0 && count > 0 && c > 0 && c % 64 == 0, "dtc_bn_fin_apply: bad shape (m=%lld count=%lld c=%d)",
                (long long)m, (long long)count, c);
  DTC_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr),
                "dtc_bn_fin_apply: running_mean and running_var go together");
  DTC_CHECK_ARG(mode == 1 || x2, "dtc_bn_fin_apply: mode %d needs x2", mode);
  BnFwdArgs a1, a2;
  a1.stats = stats; a1.count = count; a1.gamma = gamma; a1.beta = beta; a1.rmean = running_mean;
  a1.rvar = running_var; a1.nbt = nbt; a1.momentum = momentum; a1.eps = eps; a1.mean = mean; a1.invstd = invstd;
  if (mode == 3) {
    DTC_CHECK_ARG(stats2 && gamma2 && beta2 && mean2 && invstd2, "dtc_bn_fin_apply: second BN arguments");
    DTC_CHECK_ARG((running_mean2 == nullptr) == (running_var2 == nullptr),
                  "dtc_bn_fin_apply: running_mean2 and running_var2 go together");
    a2 = a1;
    a2.stats = stats2; a2.gamma = gamma2; a2.beta = beta2; a2.rmean = running_mean2; a2.rvar = running_var2;
    a2.nbt = nbt2; a2.mean = mean2; a2.invstd = invstd2;
  }
  GUARD(return bn_fin_apply(mode, x, a1, mode == 1 ? nullptr : x2, mode == 3 ? &a2 : nullptr, y, m, c, S(stream),
                            mask_bits);)
}

int dtc_bn_bwd_mask(const uint16_t* dy, const uint8_t* mask_bits, uint16_t* dz_out, const uint16_t* x1,
                    const float* gamma1, const float* mean1, const float* invstd1, float* dgamma1, float* dbeta1,
                    uint16_t* dx1, const uint16_t* x2, const float* gamma2, const float* mean2, const float* invstd2,
                    float* dgamma2, float* dbeta2, uint16_t* dx2, int64_t count, float gscale, int one_launch,
                    int64_t* acc, size_t acc_words, int64_t m, int c, void* stream) {
  DTC_CHECK_ARG(dy && mask_bits && x1 && gamma1 && mean1 && invstd1 && dx1, "dtc_bn_bwd_mask: null argument");
  DTC_CHECK_ARG(m > 0 && count > 0 && c > 0 && c % 64 == 0 && c <= 2048,
                "dtc_bn_bwd_mask: bad shape (m=%lld count=%lld c=%d)", (long long)m, (long long)count, c);
  const bool dual = x2 != nullptr;
  DTC_CHECK_ARG(!dual || (gamma2 && mean2 && invstd2 && dx2), "dtc_bn_bwd_mask: second BN arguments");
  BnBwdArgs a1, a2;
  a1.count = count; a1.gamma = gamma1; a1.mean = mean1; a1.invstd = invstd1; a1.gscale = gscale;
  a1.dgamma = dgamma1; a1.dbeta = dbeta1;
  a2 = a1;
  a2.gamma = gamma2; a2.mean = mean2; a2.invstd = invstd2; a2.dgamma = dgamma2; a2.dbeta = dbeta2;
  if (one_launch) {
    DTC_CHECK_ARG(bn_bwd_cg_ok(m, c, dual), "dtc_bn_bwd_mask: m=%lld is past the one-launch limit (%s)", (long long)m,
                  dual ? "2048 dual" : "4096");
    GUARD(return bn_bwd_cg(dy, mask_bits, dz_out, x1, a1, dx1, x2, dual ? &a2 : nullptr, dx2, m, c, S(stream));)
  }
  const size_t words = DTC_STAT_WORDS(c);
  DTC_CHECK_ARG(acc && acc_words >= (dual ? 2 : 1) * words,
                "dtc_bn_bwd_mask: the two-pass form needs %zu zeroed accumulator words", (dual ? 2 : 1) * words);
  a1.acc = acc;
  a2.acc = acc + words;
  GUARD(DTC_TRY(bn_bwd_reduce_mask(dy, mask_bits, x1, mean1, invstd1, acc, x2, mean2, invstd2,
                                   dual ? acc + words : nullptr, m, c, S(stream)));
        return bn_bwd_fin_apply_mask(dy, mask_bits, dz_out, x1, a1, dx1, x2, dual ? &a2 : nullptr, dx2, m, c,
                                     S(stream));)
}

int dtc_stem_im2col(const float* x, uint16_t* cols, int n, int h, int w, void* stream) {
  return stem_im2col(x, cols, n, h, w, S(stream));
}
int dtc_stem_pack_weight(const uint16_t* w27, uint16_t* w64, int k, void* stream) {
  return stem_pack_weight(w27, w64, k, S(stream));
}
int dtc_stem_fwd(const float* x_nchw, const uint16_t* w27, uint16_t* y, int64_t* stats, int n, int h, int w,
                 void* stream) {
  GUARD(return stem_fwd(x_nchw, w27, y, stats, n, h, w, S(stream));)
}
size_t dtc_stem_wgrad_workspace_size(int n, int h, int w) {
  return n > 0 && h > 0 && w > 0 ? stem_wgrad_slab_bytes((int64_t)n * h * w) : 0;
}
int dtc_stem_wgrad(const float* x_nchw, const uint16_t* dy, float* dw27, float scale, int n, int h, int w, void* ws,
                   size_t ws_bytes, void* stream) {
  GUARD(return stem_wgrad(x_nchw, dy, dw27, scale, n, h, w, (float*)ws, ws_bytes, S(stream));)
}
int dtc_head_fwd(const uint16_t* act, int n, int hw, int c, const uint16_t* wfc, const float* bfc, int ncls,
                 float* feat, float* logits, void* stream) {
  return head_fwd(act, n, hw, c, wfc, bfc, ncls, feat, logits, S(stream));
}
size_t dtc_head_bwd_workspace_size(int n, int c, int ncls) { return head_bwd_workspace(n, c, ncls); }
int dtc_head_bwd(const float* dlogits, const float* feat, const uint16_t* wfc, int n, int hw, int c, int ncls,
                 float scale, float* dw, float* db, uint16_t* dact, void* ws, size_t ws_bytes, void* stream) {
  return head_bwd(dlogits, feat, wfc, n, hw, c, ncls, scale, dw, db, dact, (float*)ws, ws_bytes, S(stream));
}
int dtc_xent_fwd(const float* logits, const int64_t* labels, int n, int ncls, float* loss, float* lse, void* stream) {
  return xent_fwd(logits, labels, n, ncls, loss, lse, S(stream));
}
int dtc_xent_fwd_ex(const float* logits, const int64_t* labels, int n, int ncls, float* loss, float* lse,
                    const float* scale, float* scaled, float* host_loss, void* stream) {
  GUARD(return xent_fwd_fused(logits, labels, n, ncls, loss, lse, scale, scaled, host_loss, S(stream));)
}
int dtc_xent_soft_fwd_ex(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                         float smoothing, int n, int ncls, float* loss, float* lse, const float* scale, float* scaled,
                         float* host_loss, void* stream) {
  GUARD(return xent_soft_fwd_fused(logits, labels_a, labels_b, lam, smoothing, n, ncls, loss, lse, scale, scaled,
                                   host_loss, S(stream));)
}
int dtc_xent_soft_fwd(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      float smoothing, int n, int ncls, float* loss, float* lse, void* stream) {
  GUARD(return xent_soft_fwd(logits, labels_a, labels_b, lam, smoothing, n, ncls, loss, lse, S(stream));)
}
int dtc_xent_soft_bwd(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      float smoothing, const float* lse, const float* gscale, int n, int ncls, float* dlogits,
                      void* stream) {
  GUARD(return xent_soft_bwd(logits, labels_a, labels_b, lam, smoothing, lse, gscale, n, ncls, dlogits, S(stream));)
}
int dtc_eval_metrics(const float* logits, const int64_t* labels, int n, int ncls, int topk, dtc_eval_record* rec,
                     void* stream) {
  GUARD(return eval_metrics(logits, labels, n, ncls, topk, rec, S(stream));)
}
int dtc_xent_bwd(const float* logits, const int64_t* labels, const float* lse, const float* gscale, int n, int ncls,
                 float* dlogits, void* stream) {
  return xent_bwd(logits, labels, lse, gscale, n, ncls, dlogits, S(stream));
}

int dtc_sgd_nesterov_flat(float* p, const float* g, float* mom, uint16_t* pb, int64_t n, float lr, float wd, float mu,
                          const float* inv_scale, const int* found_inf, void* stream) {
  return sgd_nesterov(p, g, mom, pb, n, lr, wd, mu, inv_scale, found_inf, S(stream));
}
int dtc_adam_state_words(void) { return DTC_ADAM_STATE_WORDS; }
int dtc_adam_flat(float* p, const float* g, float* m, float* v, uint16_t* pb, int64_t n, void* state, double lr,
                  double beta1, double beta2, double eps, double wd, int decoupled, const float* inv_scale,
                  const int* found_inf, void* stream) {
  return adam_flat(p, g, m, v, pb, n, state, lr, beta1, beta2, eps, wd, decoupled, inv_scale, found_inf, S(stream));
}
size_t dtc_grad_norm_workspace_bytes(int64_t n) { return grad_norm_workspace_bytes(n); }
int dtc_grad_norm_clip(const float* g, int64_t n, const float* inv_scale, double max_norm, void* workspace,
                       float* total_norm, float* grad_mult, void* stream) {
  return grad_norm_clip(g, n, inv_scale, max_norm, workspace, total_norm, grad_mult, S(stream));
}
static_assert(sizeof(dtc_seg) == sizeof(SegDesc) && offsetof(dtc_seg, numel) == offsetof(SegDesc, numel) &&
                  offsetof(dtc_seg, flags) == offsetof(SegDesc, flags) &&
                  offsetof(dtc_seg, reserved) == offsetof(SegDesc, reserved),
              "dtc_seg is SegDesc");
int dtc_segplan_create(dtc_segplan** out, const dtc_seg* segs, int nseg) {
  GUARD(return segplan_create((SegPlan**)out, (const SegDesc*)segs, nseg);)
}
int dtc_segplan_destroy(dtc_segplan* plan) { return segplan_destroy((SegPlan*)plan); }
int dtc_segplan_num_segments(const dtc_segplan* plan) { return segplan_num_segments((const SegPlan*)plan); }
int64_t dtc_segplan_chunk_elems(void) { return segplan_chunk_elems(); }
size_t dtc_segplan_device_bytes(const dtc_segplan* plan) { return segplan_device_bytes((const SegPlan*)plan); }
int dtc_segplan_bind(dtc_segplan* plan, void* dev, size_t bytes, void* stream) {
  return segplan_bind((SegPlan*)plan, dev, bytes, S(stream));
}
int dtc_seg_norms(dtc_segplan* plan, const float* p, const float* g, const float* gmul, float* seg_out,
                  void* stream) {
  return seg_norms((SegPlan*)plan, p, g, gmul, seg_out, S(stream));
}
int dtc_lars_flat(dtc_segplan* plan, float* p, const float* g, float* mom, uint16_t* pb, double lr, double wd,
                  double mu, int nesterov, double trust_coef, double eps, int trust_clip, const float* inv_scale,
                  const int* found_inf, float* seg_out, void* stream) {
  return lars_flat((SegPlan*)plan, p, g, mom, pb, lr, wd, mu, nesterov, trust_coef, eps, trust_clip, inv_scale,
                   found_inf, seg_out, S(stream));
}
static_assert(sizeof(dtc_ema_range) == sizeof(EmaRange) && offsetof(dtc_ema_range, src) == offsetof(EmaRange, src) &&
                  offsetof(dtc_ema_range, ema_bf16) == offsetof(EmaRange, ema_bf16) &&
                  offsetof(dtc_ema_range, n) == offsetof(EmaRange, n),
              "dtc_ema_range is EmaRange");
int dtc_ema_state_words(void) { return DTC_EMA_STATE_WORDS; }
int dtc_ema_update(const dtc_ema_range* ranges, int nranges, void* state, double decay, int warmup,
                   const int* found_inf, void* stream) {
  return ema_update((const EmaRange*)ranges, nranges, state, decay, warmup, found_inf, S(stream));
}
int dtc_grad_accum_flat(float* acc, float* g, int64_t n, int mode, void* stream) {
  return grad_accum(acc, g, n, mode, S(stream));
}
int dtc_grad_compress_bf16(const float* g, const float* acc, uint16_t* c, int64_t n, void* stream) {
  return grad_compress_bf16(g, acc, c, n, S(stream));
}
int dtc_grad_decompress_bf16(const uint16_t* c, float* g, int64_t n, void* stream) {
  return grad_decompress_bf16(c, g, n, S(stream));
}
static_assert(sizeof(dtc_psgd_tensor) == sizeof(PsgdDesc) && offsetof(dtc_psgd_tensor, rows) == offsetof(PsgdDesc, rows) &&
                  offsetof(dtc_psgd_tensor, cols) == offsetof(PsgdDesc, cols) &&
                  offsetof(dtc_psgd_tensor, rank) == offsetof(PsgdDesc, rank),
              "dtc_psgd_tensor is PsgdDesc");
int dtc_psgd_plan_create(dtc_psgd_plan** out, const dtc_psgd_tensor* tensors, int n) {
  GUARD(return psgd_plan_create((PsgdPlan**)out, (const PsgdDesc*)tensors, n);)
}
int dtc_psgd_plan_destroy(dtc_psgd_plan* plan) { return psgd_plan_destroy((PsgdPlan*)plan); }
int64_t dtc_psgd_plan_numel(const dtc_psgd_plan* plan, int what) { return psgd_plan_numel((const PsgdPlan*)plan, what); }
size_t dtc_psgd_plan_device_bytes(const dtc_psgd_plan* plan) { return psgd_plan_device_bytes((const PsgdPlan*)plan); }
int dtc_psgd_plan_bind(dtc_psgd_plan* plan, void* dev, size_t bytes, void* stream) {
  return psgd_plan_bind((PsgdPlan*)plan, dev, bytes, S(stream));
}
int dtc_psgd_orthonormalize(dtc_psgd_plan* plan, int what, float* q, float* staging, int* state, double epsilon,
                            void* stream) {
  return psgd_orthonormalize((PsgdPlan*)plan, what, q, staging, state, epsilon, S(stream));
}
int dtc_psgd_project(dtc_psgd_plan* plan, const float* g, const float* e, const float* q, float* staging,
                     void* stream) {
  return psgd_project((PsgdPlan*)plan, g, e, q, staging, S(stream));
}
int dtc_psgd_backproject(dtc_psgd_plan* plan, const float* g, const float* e, const float* staging, float* q,
                         void* stream) {
  return psgd_backproject((PsgdPlan*)plan, g, e, staging, q, S(stream));
}
int dtc_psgd_reconstruct(dtc_psgd_plan* plan, float* g, float* e, const float* staging, const float* q, int* state,
                         double c, void* stream) {
  return psgd_reconstruct((PsgdPlan*)plan, g, e, staging, q, state, c, S(stream));
}
static_assert(sizeof(dtc_sam_keep) == sizeof(SamKeep) && offsetof(dtc_sam_keep, saved) == offsetof(SamKeep, saved) &&
                  offsetof(dtc_sam_keep, bytes) == offsetof(SamKeep, bytes),
              "dtc_sam_keep is SamKeep");
int dtc_sam_state_words(void) { return DTC_SAM_STATE_WORDS; }
size_t dtc_sam_workspace_bytes(int64_t n) { return sam_workspace_bytes(n); }
int dtc_sam_perturb(float* p, const float* g, float* p_saved, uint16_t* pb, int64_t n, double rho, double eps,
                    int adaptive, const float* gmul, const dtc_sam_keep* keep, int nkeep, void* state, void* workspace,
                    void* stream) {
  return sam_perturb(p, g, p_saved, pb, n, rho, eps, adaptive, gmul, (const SamKeep*)keep, nkeep, state, workspace,
                     S(stream));
}
int dtc_sam_restore(float* p, const float* p_saved, uint16_t* pb, int64_t n, const dtc_sam_keep* keep, int nkeep,
                    const void* state, int* found_inf, void* stream) {
  return sam_restore(p, p_saved, pb, n, (const SamKeep*)keep, nkeep, state, found_inf, S(stream));
}
int dtc_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, void* stream) {
  return cast_f32_bf16(src, dst, n, S(stream));
}
int dtc_amp_scale(const float* x, const float* scale, float* out, int64_t n, void* stream) {
  return amp_scale(x, scale, out, n, S(stream));
}
int dtc_amp_check_finite(const float* g, int64_t n, int* found_inf, void* stream) {
  return amp_check_finite(g, n, found_inf, S(stream));
}
int dtc_amp_update_scale(float* scale, float* inv_scale, int* growth_tracker, int* found_inf, float growth,
                         float backoff, int interval, void* stream) {
  return amp_update_scale(scale, inv_scale, growth_tracker, found_inf, growth, backoff, interval, S(stream));
}

int dtc_cifar_augment(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                      const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                      const float* stdv, float* out, int64_t* labels, int* status, void* stream) {
  return cifar_augment(images, targets, n_images, index, crop, flip, n, h, w, pad, mean, stdv, out, labels, status,
                       S(stream));
}

int dtc_cifar_augment_mix(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                          const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                          const float* stdv, const int32_t* partner, int mode, const float* lam, const uint8_t* box,
                          float* out, int64_t* labels, int64_t* labels_b, int* status, void* stream) {
  GUARD(return cifar_augment_mix(images, targets, n_images, index, crop, flip, n, h, w, pad, mean, stdv, partner, mode,
                                 lam, box, out, labels, labels_b, status, S(stream));)
}

int dtc_cifar_augment_policy(const uint8_t* images, const int64_t* targets, int64_t n_images, const int64_t* index,
                             const uint8_t* crop, const uint8_t* flip, int n, int h, int w, int pad, const float* mean,
                             const float* stdv, const uint8_t* ops, const float* args, int n_ops, const uint8_t* erase,
                             float* out, uint8_t* out_u8, int64_t* labels, int* status, void* stream) {
  GUARD(return cifar_augment_policy(images, targets, n_images, index, crop, flip, n, h, w, pad, mean, stdv, ops, args,
                                    n_ops, erase, out, out_u8, labels, status, S(stream));)
}

size_t dtc_comm_unique_id_bytes(void) { return comm_unique_id_bytes(); }
int dtc_comm_get_unique_id(void* out) { GUARD(return comm_get_unique_id(out);) }
int dtc_comm_init(dtc_comm** out, int rank, int world, const void* id, int device) {
  GUARD(return comm_init((Comm**)out, rank, world, id, device);)
}
int dtc_comm_allreduce_sum(dtc_comm* comm, void* buf, size_t count, int dtype, void* stream) {
  return comm_allreduce((Comm*)comm, buf, count, dtype, S(stream));
}
int dtc_comm_broadcast(dtc_comm* comm, void* buf, size_t count, int dtype, int root, void* stream) {
  return comm_broadcast((Comm*)comm, buf, count, dtype, root, S(stream));
}
int dtc_comm_destroy(dtc_comm* comm) { return comm_destroy((Comm*)comm); }
int dtc_barrier(dtc_comm* comm, void* stream) { GUARD(return comm_barrier((Comm*)comm, S(stream));) }
int dtc_comm_init_loopback(dtc_comm** out, int device, int world, float factor) {
  GUARD(return comm_init_loopback((Comm**)out, device, world, factor);)
}
int dtc_comm_init_thread_group(dtc_comm** outs, int world, int device) {
  GUARD(return comm_init_thread_group((Comm**)outs, world, device);)
}
int dtc_comm_rank(const dtc_comm* comm) { return comm_rank((const Comm*)comm); }
int dtc_comm_world(const dtc_comm* comm) { return comm_world((const Comm*)comm); }
int dtc_comm_log_size(dtc_comm* comm) {
  const auto* l = comm_log((Comm*)comm);
  return l ? (int)l->size() : DTC_EINVAL;
}
int dtc_comm_log_entry(dtc_comm* comm, int idx, uint64_t* addr, uint64_t* count, int* is_async) {
  const auto* l = comm_log((Comm*)comm);
  DTC_CHECK_ARG(l && idx >= 0 && idx < (int)l->size(), "dtc_comm_log_entry: bad index");
  if (addr) *addr = (*l)[idx].addr;
  if (count) *count = (*l)[idx].count;
  if (is_async) *is_async = (*l)[idx].async;
  return 0;
}
int dtc_dp_create(dtc_dp** out, int n, const int* devices) { GUARD(return dp_create((DPGroup**)out, n, devices);) }
int dtc_dp_destroy(dtc_dp* g) { return dp_destroy((DPGroup*)g); }
int dtc_dp_is_local(const dtc_dp* g) { return dp_local((const DPGroup*)g); }
int dtc_dp_broadcast(dtc_dp* g, void* const* bufs, size_t count, int dtype, void* const* streams) {
  GUARD(return dp_broadcast((DPGroup*)g, bufs, count, dtype, streams);)
}
int dtc_dp_reduce_add(dtc_dp* g, float* const* bufs, size_t count, void* const* streams) {
  GUARD(return dp_reduce_add((DPGroup*)g, bufs, count, streams);)
}
int dtc_copy_peer(void* dst, int dst_device, const void* src, int src_device, size_t bytes, void* stream) {
  return copy_peer(dst, dst_device, src, src_device, bytes, S(stream));
}
int dtc_comm_log_clear(dtc_comm* comm) {
  DTC_CHECK_ARG(comm != nullptr, "dtc_comm_log_clear: null comm");
  comm_log_clear((Comm*)comm);
  return 0;
}

}  // extern "C"
