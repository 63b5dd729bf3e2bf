// dvh_sizing.cpp -- reliability sizing on the GPU (include/dervet_hip.h: dvh_outage_first_uncovered,
// dvh_sizing_windows, dvh_size_reliability, dvh_last_sizing_ms).
//
// Replaces the cutting-plane loop of Reliability.sizing_module (dervet/MicrogridValueStreams/Reliability.py:153-219):
// its sizing program (size_for_outages :221-274, GLPK_MI) becomes an LP built on the device from the resident series
// (dvh_sizing.hip) and solved with every other unfinished case's in one batched PDHG solve; its serial scan
// (find_first_uncovered :391-445, 8,760 Python simulations per round) becomes one launch of the outage kernel's
// first-uncovered mode (dvh_outage.hip).  The series are uploaded once; per round only the case structs, the LP
// descriptors and a few words per case cross the bus.
#include <cmath>
#include <numeric>
#include <string>

#include "dvh_host.h"
#include "dvh_sizing_validate.h"

namespace dvh {

struct SizingBuf : DevBuf {
  SizingBuf() { slack_div = 4; }  // the LPs grow by one window per round
};

struct SizingState {
  SizingBuf series, cases, lps, starts, desc, indptr, indices, data, c, c0, q, l, u, x, y, stats, istats, sizes, first,
      count;
  DevEvent ev[4];  // whole call; the phase being timed
  double ms = 0.0, out3[3] = {0.0, 0.0, 0.0};
};

void sizing_destroy(SizingState* s) { delete s; }

}  // namespace dvh

namespace {

using dvh::HandleView;
using dvh::SizingState;

// The handle's sizing state, created on first use (on the handle's device).
int state(const HandleView& v, SizingState** out) {
  DVH_VIEW_HIP(v, hipSetDevice(v.device));
  if (!*v.sizing) *v.sizing = new SizingState();
  *out = *v.sizing;
  for (DevEvent& e : (*out)->ev) DVH_VIEW_HIP(v, e.ensure());
  return DVH_OK;
}

// Every case's series to the device, once; oc[k] = the kernel's case struct with device pointers, simulating
// steps[k] steps from soe0 (init_soe dropped: the sizing scan starts every outage from soe0).
int upload_series(const HandleView& v, SizingState* st, const dvh_outage_case* cases, int count,
                  const std::vector<int>& steps, std::vector<dvh::OutageCase>& oc) {
  std::vector<double> data = dvh::outage_stage(cases, count, false);
  DVH_VIEW_HIP(v, st->series.ensure(sizeof(double) * data.size()));
  oc.resize(count);
  dvh::outage_stage_fill(cases, count, false, data, st->series.as<double>(), oc.data());
  for (int k = 0; k < count; ++k) oc[k].outage_len = steps[k];
  DVH_VIEW_HIP(v, hipMemcpyAsync(st->series.p, data.data(), sizeof(double) * data.size(), hipMemcpyHostToDevice,
                                 v.stream));
  DVH_VIEW_HIP(v, hipStreamSynchronize(v.stream));  // the staging vector ends here
  return DVH_OK;
}

// The scan over the listed cases (structs uploaded compactly): first[i] = -1 when every start is covered.
int scan(const HandleView& v, SizingState* st, const std::vector<dvh::OutageCase>& oc, const std::vector<int>& list,
         std::vector<int32_t>& first, std::vector<int32_t>& nunc) {
  const int n = (int)list.size();
  first.assign(n, INT32_MAX);
  nunc.assign(n, 0);
  if (n == 0) return DVH_OK;
  std::vector<dvh::OutageCase> sel(n);
  int max_n = 0;
  for (int i = 0; i < n; ++i) {
    sel[i] = oc[list[i]];
    max_n = std::max(max_n, sel[i].n_steps);
  }
  DVH_VIEW_HIP(v, st->cases.ensure(sizeof(dvh::OutageCase) * n));
  DVH_VIEW_HIP(v, st->first.ensure(sizeof(int32_t) * n));
  DVH_VIEW_HIP(v, st->count.ensure(sizeof(int32_t) * n));
  hipStream_t s = v.stream;
  DVH_VIEW_HIP(v, hipMemcpyAsync(st->cases.p, sel.data(), sizeof(dvh::OutageCase) * n, hipMemcpyHostToDevice, s));
  DVH_VIEW_HIP(v, hipMemcpyAsync(st->first.p, first.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
  DVH_VIEW_HIP(v, hipMemsetAsync(st->count.p, 0, sizeof(int32_t) * n, s));
  DVH_VIEW_HIP(v, hipEventRecord(st->ev[2], s));
  hipError_t e = dvh::launch_outage_first_uncovered(st->cases.as<dvh::OutageCase>(), n, max_n, st->first.as<int32_t>(),
                                                    st->count.as<int32_t>(), s);
  if (e != hipSuccess) return fail(v, DVH_ERR_HIP, std::string("launch_outage_first_uncovered: ") + hipGetErrorString(e));
  DVH_VIEW_HIP(v, hipEventRecord(st->ev[3], s));
  DVH_VIEW_HIP(v, hipMemcpyAsync(first.data(), st->first.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  DVH_VIEW_HIP(v, hipMemcpyAsync(nunc.data(), st->count.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  DVH_VIEW_HIP(v, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, st->ev[2], st->ev[3]) == hipSuccess) st->out3[1] += ms;
  for (int i = 0; i < n; ++i)
    if (nunc[i] == 0) first[i] = -1;
  return DVH_OK;
}

dvh::SizingLP lp_of(const dvh::OutageCase& o, const dvh_sizing_spec& s, int L) {
  dvh::SizingLP p{};
  p.cl = o.critical_load;
  p.pv_vari = o.pv_vari;
  p.shed = o.load_shed;
  p.n_steps = o.n_steps;
  p.L = L;
  p.new_start = -1;
  p.dt = o.dt;
  p.dg_gen = o.dg_gen;
  p.rte = o.rte;
  p.llsoc = s.llsoc;
  p.ulsoc = s.ulsoc;
  p.a0 = std::min(s.soc_init, s.ulsoc);
  p.lE = s.size_energy ? s.energy_min : s.energy;
  p.uE = s.size_energy ? s.energy_max : s.energy;
  p.lP = s.size_power ? s.power_min : s.power;
  p.uP = s.size_power ? s.power_max : s.power;
  p.cE = s.ccost_kwh;
  p.cP = s.ccost_kw;
  p.c0 = s.ccost;
  return p;
}

// Descriptors and device arrays of the LPs `lps` (windows 0 .. n - 1 of a packed batch), built on the device.
int build_batch(const HandleView& v, SizingState* st, const std::vector<dvh::SizingLP>& lps,
                std::vector<int64_t>& desc, dvh_packed& bt) {
  const int n = (int)lps.size();
  desc.assign(8 * (size_t)n, 0);
  int64_t tn = 0, tm = 0, tz = 0, tr = 0;
  for (int b = 0; b < n; ++b) {
    const int64_t KL = (int64_t)lps[b].K * lps[b].L;
    int64_t* d = &desc[8 * (size_t)b];
    d[0] = 2 + 3 * KL;
    d[1] = 6 * KL;
    d[2] = KL;
    d[3] = 14 * KL;
    d[4] = tr;
    d[5] = tz;
    d[6] = tn;
    d[7] = tm;
    tr += d[1] + 1;
    tz += d[3];
    tn += d[0];
    tm += d[1];
  }
  const size_t D = sizeof(double), I = sizeof(int32_t);
  DVH_VIEW_HIP(v, st->desc.ensure(desc.size() * sizeof(int64_t)));
  DVH_VIEW_HIP(v, st->lps.ensure(sizeof(dvh::SizingLP) * n));
  DVH_VIEW_HIP(v, st->indptr.ensure(I * tr));
  DVH_VIEW_HIP(v, st->indices.ensure(I * tz));
  DVH_VIEW_HIP(v, st->data.ensure(D * tz));
  DVH_VIEW_HIP(v, st->c.ensure(D * tn));
  DVH_VIEW_HIP(v, st->l.ensure(D * tn));
  DVH_VIEW_HIP(v, st->u.ensure(D * tn));
  DVH_VIEW_HIP(v, st->x.ensure(D * tn));
  DVH_VIEW_HIP(v, st->q.ensure(D * tm));
  DVH_VIEW_HIP(v, st->y.ensure(D * tm));
  DVH_VIEW_HIP(v, st->c0.ensure(D * n));
  DVH_VIEW_HIP(v, st->stats.ensure(D * 4 * n));
  DVH_VIEW_HIP(v, st->istats.ensure(I * 2 * n));
  DVH_VIEW_HIP(v, st->sizes.ensure(D * 4 * n));
  hipStream_t s = v.stream;
  DVH_VIEW_HIP(v, hipMemcpyAsync(st->desc.p, desc.data(), desc.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
  DVH_VIEW_HIP(v, hipMemcpyAsync(st->lps.p, lps.data(), sizeof(dvh::SizingLP) * n, hipMemcpyHostToDevice, s));
  hipError_t e = dvh::launch_build_sizing(st->lps.as<dvh::SizingLP>(), n, st->desc.as<int64_t>(),
                                          st->indptr.as<int32_t>(), st->indices.as<int32_t>(), st->data.as<double>(),
                                          st->c.as<double>(), st->c0.as<double>(), st->q.as<double>(),
                                          st->l.as<double>(), st->u.as<double>(), s);
  if (e != hipSuccess) return fail(v, DVH_ERR_HIP, std::string("launch_build_sizing: ") + hipGetErrorString(e));
  DVH_VIEW_HIP(v, hipStreamSynchronize(s));  // desc and lps are the caller's vectors
  bt = dvh_packed{n, 0, tn, tm, tz, tr, st->desc.as<int64_t>(), st->indptr.as<int32_t>(), st->indices.as<int32_t>(),
                  st->data.as<double>(), st->c.as<double>(), st->c0.as<double>(), st->q.as<double>(),
                  st->l.as<double>(), st->u.as<double>(), st->x.as<double>(), st->y.as<double>(),
                  st->stats.as<double>(), st->istats.as<int32_t>()};
  return DVH_OK;
}

// The per-case device regions of the outage starts (capacity cap[k]), filled with the given starts.
int upload_starts(const HandleView& v, SizingState* st, const std::vector<std::vector<int32_t>>& S,
                  const std::vector<int>& cap, std::vector<int32_t*>& region) {
  const int count = (int)S.size();
  size_t total = 0;
  for (int k = 0; k < count; ++k) total += (size_t)cap[k];
  DVH_VIEW_HIP(v, st->starts.ensure(sizeof(int32_t) * total));
  std::vector<int32_t> flat(total, 0);
  region.assign(count, nullptr);
  size_t off = 0;
  for (int k = 0; k < count; ++k) {
    std::copy(S[k].begin(), S[k].end(), flat.begin() + off);
    region[k] = st->starts.as<int32_t>() + off;
    off += (size_t)cap[k];
  }
  DVH_VIEW_HIP(v, hipMemcpyAsync(st->starts.p, flat.data(), sizeof(int32_t) * total, hipMemcpyHostToDevice, v.stream));
  DVH_VIEW_HIP(v, hipStreamSynchronize(v.stream));
  return DVH_OK;
}

// ceil(x - delta) (up: ceil(x + delta)), delta = 1e-7 max(1, |x|), floored at the lower bound
double candidate(double x, double lo, bool up) {
  const double d = 1e-7 * std::max(1.0, std::fabs(x));
  return std::max(std::ceil(up ? x + d : x - d), lo);
}

// Restores the handle's options on every way out of dvh_size_reliability.
struct OptionsGuard {
  dvh_options* o;
  dvh_options saved;
  explicit OptionsGuard(dvh_options* p) : o(p), saved(*p) {}
  ~OptionsGuard() { *o = saved; }
};

}  // namespace

extern "C" {

int dvh_outage_first_uncovered(dvh_handle* h, const dvh_outage_case* cases, int32_t count, const int32_t* target_steps,
                               int32_t* first, int32_t* n_uncovered) {
  if (!h) return DVH_ERR_ARG;
  const HandleView v = dvh::handle_view(h);
  std::string msg = dvh::validate_scan(cases, count, target_steps);
  if (msg.empty() && count > 0 && (!first || !n_uncovered)) msg = "first and n_uncovered are required";
  if (!msg.empty()) return fail(v, DVH_ERR_ARG, msg);
  if (count == 0) return DVH_OK;
  SizingState* st = nullptr;
  if (int rc = state(v, &st)) return rc;
  std::vector<dvh::OutageCase> oc;
  if (int rc = upload_series(v, st, cases, count, std::vector<int>(target_steps, target_steps + count), oc)) return rc;
  std::vector<int> all(count);
  std::iota(all.begin(), all.end(), 0);
  std::vector<int32_t> f, n;
  if (int rc = scan(v, st, oc, all, f, n)) return rc;
  std::copy(f.begin(), f.end(), first);
  std::copy(n.begin(), n.end(), n_uncovered);
  return DVH_OK;
}

int dvh_sizing_windows(dvh_handle* h, const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count,
                       const int32_t* starts, const int32_t* n_starts, dvh_result* out) {
  if (!h) return DVH_ERR_ARG;
  const HandleView v = dvh::handle_view(h);
  std::string msg = dvh::validate_sizing(cases, specs, count);
  if (msg.empty()) msg = dvh::validate_starts(cases, specs, count, starts, n_starts);
  if (msg.empty() && count > 0 && !out) msg = "out is required";
  if (!msg.empty()) return fail(v, DVH_ERR_ARG, msg);
  if (count == 0) return DVH_OK;
  SizingState* st = nullptr;
  if (int rc = state(v, &st)) return rc;
  std::vector<int> L(count), cap(count);
  std::vector<std::vector<int32_t>> S(count);
  size_t off = 0;
  for (int k = 0; k < count; ++k) {
    L[k] = dvh::sizing_steps(cases[k], specs[k]);
    S[k].assign(starts + off, starts + off + n_starts[k]);
    cap[k] = n_starts[k];
    off += n_starts[k];
  }
  std::vector<dvh::OutageCase> oc;
  if (int rc = upload_series(v, st, cases, count, L, oc)) return rc;
  std::vector<int32_t*> region;
  if (int rc = upload_starts(v, st, S, cap, region)) return rc;
  std::vector<dvh::SizingLP> lps(count);
  for (int k = 0; k < count; ++k) {
    lps[k] = lp_of(oc[k], specs[k], L[k]);
    lps[k].K = n_starts[k];
    lps[k].starts = region[k];
  }
  std::vector<int64_t> desc;
  dvh_packed bt;
  if (int rc = build_batch(v, st, lps, desc, bt)) return rc;
  if (int rc = dvh_solve_packed_device(h, &bt, nullptr)) return rc;
  std::vector<double> stats(4 * (size_t)count);
  std::vector<int32_t> ist(2 * (size_t)count);
  hipStream_t s = v.stream;
  DVH_VIEW_HIP(v, hipMemcpyAsync(stats.data(), st->stats.p, sizeof(double) * stats.size(), hipMemcpyDeviceToHost, s));
  DVH_VIEW_HIP(v, hipMemcpyAsync(ist.data(), st->istats.p, sizeof(int32_t) * ist.size(), hipMemcpyDeviceToHost, s));
  for (int k = 0; k < count; ++k) {
    const int64_t* d = &desc[8 * (size_t)k];
    if (out[k].x)
      DVH_VIEW_HIP(v, hipMemcpyAsync(out[k].x, st->x.as<double>() + d[6], sizeof(double) * d[0], hipMemcpyDeviceToHost,
                                     s));
    if (out[k].y)
      DVH_VIEW_HIP(v, hipMemcpyAsync(out[k].y, st->y.as<double>() + d[7], sizeof(double) * d[1], hipMemcpyDeviceToHost,
                                     s));
  }
  DVH_VIEW_HIP(v, hipStreamSynchronize(s));
  for (int k = 0; k < count; ++k) {
    dvh_result& r = out[k];
    r.obj = stats[4 * k];
    r.primal_res_rel = stats[4 * k + 1];
    r.dual_res_rel = stats[4 * k + 2];
    r.gap_rel = stats[4 * k + 3];
    r.status = ist[2 * k];
    r.iters = ist[2 * k + 1];
  }
  return DVH_OK;
}

int dvh_size_reliability(dvh_handle* h, const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count,
                         dvh_sizing_result* out) {
  if (!h) return DVH_ERR_ARG;
  const HandleView v = dvh::handle_view(h);
  std::string msg = dvh::validate_sizing(cases, specs, count);
  if (msg.empty() && count > 0 && !out) msg = "out is required";
  if (!msg.empty()) return fail(v, DVH_ERR_ARG, msg);
  if (count == 0) return DVH_OK;
  SizingState* st = nullptr;
  if (int rc = state(v, &st)) return rc;
  st->ms = st->out3[0] = st->out3[1] = st->out3[2] = 0.0;
  hipStream_t s = v.stream;
  DVH_VIEW_HIP(v, hipEventRecord(st->ev[0], s));

  // ---- seeds: the first n_seed starts of a stable descending sort of the rolling requirement
  std::vector<int> L(count), cap(count);
  std::vector<std::vector<int32_t>> S(count);
  for (int k = 0; k < count; ++k) {
    const dvh_outage_case& c = cases[k];
    L[k] = dvh::sizing_steps(c, specs[k]);
    cap[k] = specs[k].n_seed + specs[k].max_rounds;
    const int N = c.n_steps;
    std::vector<double> req(N);
    for (int t = 0; t < N; ++t) {
      double a = 0.0;
      for (int j = 0; j < L[k] && t + j < N; ++j) a = a + c.critical_load[t + j];
      req[t] = a * c.dt;
    }
    std::vector<int32_t> idx(N);
    std::iota(idx.begin(), idx.end(), 0);
    // (ties broken by the index: the order of a stable descending sort, without sorting the whole series)
    const int ns = std::min(N, specs[k].n_seed);
    std::partial_sort(idx.begin(), idx.begin() + ns, idx.end(),
                      [&](int32_t a, int32_t b) { return req[a] > req[b] || (req[a] == req[b] && a < b); });
    S[k].assign(idx.begin(), idx.begin() + ns);
  }
  std::vector<dvh::OutageCase> oc;
  if (int rc = upload_series(v, st, cases, count, L, oc)) return rc;
  std::vector<int32_t*> region;
  if (int rc = upload_starts(v, st, S, cap, region)) return rc;
  std::vector<dvh::SizingLP> lp(count);
  for (int k = 0; k < count; ++k) {
    lp[k] = lp_of(oc[k], specs[k], L[k]);
    lp[k].starts = region[k];
    out[k].energy = out[k].power = out[k].capex = 0.0;
    out[k].status = DVH_SIZING_ROUND_LIMIT;
    out[k].lp_status = -1;
    out[k].rounds = out[k].lp_iters = 0;
    out[k].reserved = 0;
  }

  // ---- for this call the LPs are solved to eps = eps_obj = 1e-8 at least (the objective-error test, an extra
  // condition, is switched on when the handle has it off): the candidate rounds the optimum to an integer
  OptionsGuard guard(v.opts);
  v.opts->eps = std::min(guard.saved.eps, 1e-8);
  v.opts->eps_obj = guard.saved.eps_obj > 0.0 ? std::min(guard.saved.eps_obj, 1e-8) : 1e-8;

  std::vector<int> act(count);
  std::iota(act.begin(), act.end(), 0);
  std::vector<int32_t> pending(count, -1);  // the start found last round, stored by this round's build
  auto set_candidate = [&](int k, double xe, double xp, bool up) {
    const dvh_sizing_spec& sp = specs[k];
    const double E = sp.size_energy ? candidate(xe, sp.energy_min, up) : sp.energy;
    const double P = sp.size_power ? candidate(xp, sp.power_min, up) : sp.power;
    out[k].energy = E;
    out[k].power = P;
    dvh::OutageCase& o = oc[k];
    o.soe0 = sp.soc_init * E;
    o.soe_min = sp.llsoc * E;
    o.soe_max = sp.ulsoc * E;
    o.charge_max = P;
    o.discharge_max = P;
  };
  while (!act.empty()) {
    const int na = (int)act.size();
    // (1) the LPs of the unfinished cases, built on the device and solved in one batch
    std::vector<dvh::SizingLP> lps(na);
    for (int i = 0; i < na; ++i) {
      const int k = act[i];
      lp[k].K = (int)S[k].size();
      lp[k].new_start = pending[k];
      pending[k] = -1;
      lps[i] = lp[k];
    }
    std::vector<int64_t> desc;
    dvh_packed bt;
    DVH_VIEW_HIP(v, hipEventRecord(st->ev[2], s));
    if (int rc = build_batch(v, st, lps, desc, bt)) return rc;
    if (int rc = dvh_solve_packed_device(h, &bt, nullptr)) return rc;
    hipError_t e = dvh::launch_gather_sizes(st->desc.as<int64_t>(), st->x.as<double>(), st->istats.as<int32_t>(), na,
                                            st->sizes.as<double>(), s);
    if (e != hipSuccess) return fail(v, DVH_ERR_HIP, std::string("launch_gather_sizes: ") + hipGetErrorString(e));
    DVH_VIEW_HIP(v, hipEventRecord(st->ev[3], s));
    std::vector<double> sizes(4 * (size_t)na);
    DVH_VIEW_HIP(v, hipMemcpyAsync(sizes.data(), st->sizes.p, sizeof(double) * sizes.size(), hipMemcpyDeviceToHost, s));
    DVH_VIEW_HIP(v, hipStreamSynchronize(s));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, st->ev[2], st->ev[3]) == hipSuccess) st->out3[0] += ms;
    // (2), (3) candidates and their limits
    std::vector<int> live;
    for (int i = 0; i < na; ++i) {
      const int k = act[i];
      out[k].rounds += 1;
      out[k].lp_status = (int32_t)sizes[4 * i + 2];
      out[k].lp_iters += (int32_t)sizes[4 * i + 3];
      st->out3[2] += 1.0;
      if (out[k].lp_status != DVH_OPTIMAL) {
        out[k].status = DVH_SIZING_LP_FAILED;
        continue;
      }
      set_candidate(k, sizes[4 * i], sizes[4 * i + 1], false);
      live.push_back(i);
    }
    // (4), (5) the scan; a start already in the LP: once more with the candidate rounded up from x + delta
    std::vector<int> list;
    for (int i : live) list.push_back(act[i]);
    std::vector<int32_t> first, nunc;
    if (int rc = scan(v, st, oc, list, first, nunc)) return rc;
    std::vector<int> again, next;
    auto known = [&](int k, int32_t t) { return std::find(S[k].begin(), S[k].end(), t) != S[k].end(); };
    auto settle = [&](int k, int32_t f) {  // f: an uncovered start not yet in the LP, or -1
      if (f < 0) {
        out[k].status = DVH_SIZING_SIZED;
      } else if (out[k].rounds >= specs[k].max_rounds) {
        out[k].status = DVH_SIZING_ROUND_LIMIT;
      } else {
        S[k].push_back(f);
        pending[k] = f;
        next.push_back(k);
      }
    };
    for (size_t j = 0; j < list.size(); ++j) {
      const int k = list[j];
      if (first[j] >= 0 && known(k, first[j])) {
        const int i = live[j];
        set_candidate(k, sizes[4 * i], sizes[4 * i + 1], true);
        again.push_back(k);
      } else {
        settle(k, first[j]);
      }
    }
    if (!again.empty()) {
      if (int rc = scan(v, st, oc, again, first, nunc)) return rc;
      for (size_t j = 0; j < again.size(); ++j) {
        const int k = again[j];
        if (first[j] >= 0 && known(k, first[j])) out[k].status = DVH_SIZING_STALLED;
        else settle(k, first[j]);
      }
    }
    std::sort(next.begin(), next.end());
    act.swap(next);
  }
  for (int k = 0; k < count; ++k) {
    const dvh_sizing_spec& sp = specs[k];
    out[k].capex = sp.ccost + sp.ccost_kw * out[k].power + sp.ccost_kwh * out[k].energy;
    out[k].n_starts = (int32_t)S[k].size();
    if (out[k].starts) std::copy(S[k].begin(), S[k].end(), out[k].starts);
  }
  DVH_VIEW_HIP(v, hipEventRecord(st->ev[1], s));
  DVH_VIEW_HIP(v, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, st->ev[0], st->ev[1]) == hipSuccess) st->ms = ms;
  return DVH_OK;
}

int dvh_last_sizing_ms(const dvh_handle* h, double* ms, double* out3) {
  if (!h || !ms) return DVH_ERR_ARG;
  const HandleView v = dvh::handle_view(const_cast<dvh_handle*>(h));
  const SizingState* st = *v.sizing;
  *ms = st ? st->ms : 0.0;
  if (out3)
    for (int i = 0; i < 3; ++i) out3[i] = st ? st->out3[i] : 0.0;
  return DVH_OK;
}

}  // extern "C"
