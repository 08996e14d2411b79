// ResNet-18 executor, measurement: the per-call profiling slots and event brackets behind the PROF macro,
// the communication timers of a backward with a communicator, and the entry points that arm and read them.
#include <algorithm>
#include "net.h"

namespace dtc {

u64* prof_slot(Net& n, int kind, double flops) {
  ProfState& p = n.prof;
  if (!p.on || p.next >= ProfState::SLOTS) return nullptr;
  const int i = p.next++;
  p.kind[i] = kind;
  p.flops[i] = flops;
  return p.ts + (size_t)i * DTC_PROF_SLOT_U64;
}

int prof_ev_open(Net& n, int kind, double work) {
  ProfState& p = n.prof;
  // (p.st may be the null stream: the caller's default stream)
  if (!p.on || !p.events || n.graph.cap_locked || side_on()) return -1;
  if (p.evn * 2 + 1 >= p.evpool.size()) {  // pool used up: counted, so the caller can refuse the total
    ++p.evdropped;
    return -1;
  }
  const int i = (int)p.evn++;
  if (p.evwork.size() < p.evn) p.evwork.resize(p.evn);
  p.evwork[i] = {kind, work};
  if (hipEventRecord(p.evpool[2 * i], p.st) != hipSuccess) return -1;
  return i;
}

void prof_ev_close(Net& n, int i) {
  if (i >= 0) (void)hipEventRecord(n.prof.evpool[2 * i + 1], n.prof.st);
}

void ct_free(Net& n) {
  for (auto& c : n.ct.steps) {
    for (hipEvent_t e : {c.bwd0, c.join_c, c.join_d, c.tail_a, c.tail_b})
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c.b0) (void)hipEventDestroy(e);
    for (hipEvent_t e : c.b1) (void)hipEventDestroy(e);
  }
  n.ct.steps.clear();
  n.ct.left = n.ct.used = 0;
}

static void zero_kinds(int nkinds, double* ms, double* work, int* count) {
  for (int k = 0; k < nkinds; ++k) {
    if (ms) ms[k] = 0;
    if (work) work[k] = 0;
    if (count) count[k] = 0;
  }
}

}  // namespace dtc

// ------------------------------------------------------------------ C ABI (profiling and communication timing)
using namespace dtc;

extern "C" {

int dtc_rn18_profile_begin(dtc_net* net, int capacity) {
  DTC_CHECK_ARG(net && capacity > 0 && net->n.mem.ws, "dtc_rn18_profile_begin: bad args or unbound net");
  ProfState& p = net->n.prof;
  const size_t bytes = (size_t)ProfState::SLOTS * 2 * sizeof(u64);
  const size_t ts_bytes = (size_t)ProfState::SLOTS * DTC_PROF_SLOT_U64 * sizeof(u64);
  int dev = 0;
  DTC_HIP(hipGetDevice(&dev));
  DTC_HIP(hipDeviceGetAttribute(&p.khz, hipDeviceAttributeWallClockRate, dev));
  DTC_CHECK_ARG(p.khz > 0, "dtc_rn18_profile_begin: no wall clock rate");
  // the previous step may still run (its profiled graphs stamp these slots): drain, then reset.
  // slots -> (~0, 0) (folding all-zero slots adds nothing and resets them), then totals -> 0.
  // The drains hold g_graph_mu like drop_graphs: no device drain while another host
  // thread's stream is capturing.
  std::lock_guard<std::recursive_mutex> lk(g_graph_mu);
  DTC_HIP(hipDeviceSynchronize());
  DTC_HIP(hipMemset(p.ts, 0, ts_bytes));
  DTC_TRY(prof_accumulate(p.ts, ProfState::SLOTS, p.acc, nullptr));
  DTC_HIP(hipMemset(p.acc, 0, bytes));
  DTC_HIP(hipDeviceSynchronize());
  p.on = true;  // the next calls launch (capturing on first use) the profiled graph set
  return 0;
}

int dtc_rn18_profile_events(dtc_net* net, int pairs) {
  DTC_CHECK_ARG(net && pairs >= 0, "dtc_rn18_profile_events: bad args");
  ProfState& p = net->n.prof;
  p.events = pairs > 0;
  p.evn = 0;
  p.evdropped = 0;
  const size_t want = (size_t)pairs * 2;
  while (p.evpool.size() < want) {
    hipEvent_t e;
    // timing events without the system-scope release fence at completion (no L2 write-back between the
    // bracketed launches: the kernels see the caches the unbracketed step gives them)
    DTC_HIP(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    p.evpool.push_back(e);
  }
  return 0;
}

int dtc_rn18_profile_events_result(dtc_net* net, int nkinds, double* ms_by_kind, double* work_by_kind,
                                   int* count_by_kind) {
  DTC_CHECK_ARG(net != nullptr && nkinds >= 1 && nkinds <= 4, "dtc_rn18_profile_events_result: bad args");
  ProfState& p = net->n.prof;
  zero_kinds(nkinds, ms_by_kind, work_by_kind, count_by_kind);
  for (size_t i = 0; i < p.evn; ++i) {
    const int k = p.evwork[i].first;
    if (k >= nkinds) continue;
    DTC_HIP(hipEventSynchronize(p.evpool[2 * i + 1]));
    float ms = 0.f;
    DTC_HIP(hipEventElapsedTime(&ms, p.evpool[2 * i], p.evpool[2 * i + 1]));
    if (ms_by_kind) ms_by_kind[k] += ms;
    if (work_by_kind) work_by_kind[k] += p.evwork[i].second;
    if (count_by_kind) count_by_kind[k] += 1;
  }
  p.evn = 0;
  p.events = false;
  return 0;
}

int dtc_rn18_profile_events_dropped(dtc_net* net, long long* dropped) {
  DTC_CHECK_ARG(net != nullptr && dropped != nullptr, "dtc_rn18_profile_events_dropped: bad args");
  *dropped = net->n.prof.evdropped;
  return 0;
}

int dtc_rn18_profile_end_ex(dtc_net* net, int nkinds, double* ms_by_kind, double* work_by_kind, int* count_by_kind) {
  DTC_CHECK_ARG(net != nullptr && nkinds >= 1 && nkinds <= 4, "dtc_rn18_profile_end_ex: bad args");
  ProfState& p = net->n.prof;
  zero_kinds(nkinds, ms_by_kind, work_by_kind, count_by_kind);
  if (!p.on) return 0;
  std::vector<u64> acc((size_t)ProfState::SLOTS * 2);
  std::lock_guard<std::recursive_mutex> lk(g_graph_mu);  // as profile_begin
  DTC_HIP(hipDeviceSynchronize());
  DTC_HIP(hipMemcpy(acc.data(), p.acc, acc.size() * sizeof(u64), hipMemcpyDeviceToHost));
  for (int i = 0; i < ProfState::SLOTS; ++i) {
    const u64 calls = acc[2 * i + 1];
    if (calls == 0) continue;
    const int k = p.kind[i];
    if (k >= nkinds) continue;
    if (ms_by_kind) ms_by_kind[k] += (double)acc[2 * i] / (double)p.khz;
    if (work_by_kind) work_by_kind[k] += p.flops[i] * (double)calls;
    if (count_by_kind) count_by_kind[k] += (int)calls;
  }
  p.on = false;  // back to the plain graph set; both sets stay captured
  return 0;
}

int dtc_rn18_profile_end(dtc_net* net, double* ms_by_kind, double* flops_by_kind, int* count_by_kind) {
  return dtc_rn18_profile_end_ex(net, 3, ms_by_kind, flops_by_kind, count_by_kind);
}

int dtc_rn18_comm_timing(dtc_net* net, int steps) {
  DTC_CHECK_ARG(net && steps >= 0 && steps <= 100000, "dtc_rn18_comm_timing: bad args");
  Net& n = net->n;
  ct_free(n);
  const size_t nb = n.plan.bucket_off.size();
  n.ct.steps.resize(steps);
  for (auto& c : n.ct.steps) {
    for (hipEvent_t* e : {&c.bwd0, &c.join_c, &c.join_d, &c.tail_a, &c.tail_b}) DTC_HIP(hipEventCreate(e));
    c.b0.resize(nb);
    c.b1.resize(nb);
    for (size_t i = 0; i < nb; ++i) {
      DTC_HIP(hipEventCreate(&c.b0[i]));
      DTC_HIP(hipEventCreate(&c.b1[i]));
    }
  }
  n.ct.left = steps;
  return 0;
}

int dtc_rn18_comm_timing_result(dtc_net* net, int max_buckets, double* bucket_us, double* exposed_us, int* steps) {
  DTC_CHECK_ARG(net && max_buckets >= 0 && (max_buckets == 0 || bucket_us) && exposed_us && steps,
                "dtc_rn18_comm_timing_result: bad args");
  Net& n = net->n;
  const int nb = std::min<int>(max_buckets, (int)n.plan.bucket_off.size());
  for (int i = 0; i < 3 * max_buckets; ++i) bucket_us[i] = 0.0;
  for (int i = 0; i < 5; ++i) exposed_us[i] = 0.0;
  auto us = [](hipEvent_t a, hipEvent_t b, double& out) -> int {
    float ms = 0.f;
    DTC_HIP(hipEventSynchronize(b));
    DTC_HIP(hipEventElapsedTime(&ms, a, b));
    out = 1e3 * (double)ms;
    return 0;
  };
  int recorded = 0, joined = 0, tailed = 0;
  std::vector<int> bcount(nb, 0);
  for (int k = 0; k < n.ct.used; ++k) {
    CommTimes& c = n.ct.steps[k];
    if (!c.ok) continue;  // a backward that failed recorded no end event
    double bwd = 0;
    if (c.tail) {  // (a replayed backward records no tail / join events)
      double tail = 0;
      DTC_TRY(us(c.tail_a, c.tail_b, tail));
      exposed_us[0] += tail;
      ++tailed;
    }
    DTC_TRY(us(c.bwd0, c.tail_b, bwd));
    exposed_us[3] += bwd;
    if (c.join) {
      double j = 0;
      DTC_TRY(us(c.join_c, c.join_d, j));
      exposed_us[1] += j;
      ++joined;
    }
    for (int i = 0; i < nb; ++i) {
      if (!c.bucket[i]) continue;
      double a = 0, b = 0;
      DTC_TRY(us(c.bwd0, c.b0[i], a));
      DTC_TRY(us(c.bwd0, c.b1[i], b));
      bucket_us[3 * i] += a;
      bucket_us[3 * i + 1] += b;
      bucket_us[3 * i + 2] += b - a;
      ++bcount[i];
    }
    ++recorded;
  }
  // tail: the mean over the steps that recorded one, -1 when none did (replayed backwards: unavailable)
  exposed_us[0] = tailed ? exposed_us[0] / tailed : -1.0;
  if (recorded) exposed_us[3] /= recorded;
  if (joined) exposed_us[1] /= joined;
  exposed_us[2] = tailed ? exposed_us[0] + exposed_us[1] : -1.0;
  exposed_us[4] = joined;
  for (int i = 0; i < nb; ++i)
    if (bcount[i])
      for (int j = 0; j < 3; ++j) bucket_us[3 * i + j] /= bcount[i];
  *steps = recorded;
  ct_free(n);
  return 0;
}

}  // extern "C"
