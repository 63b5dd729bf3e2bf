// dvh_solve.cpp -- the solve entry points of the C ABI (include/dervet_hip.h).
//
// Replaces the per-window solve of storagevet Scenario.solve_optimization (dervet/MicrogridScenario.py:319)
// for a whole batch of windows: validates and packs host LPs, moves them to HBM, runs the setup and PDHG
// kernels chunk by chunk on the handle's stream, and copies primal/dual solutions and statistics back.
#include <chrono>
#include <thread>

#include "dvh_handle.h"
#include "dvh_validate.h"

namespace {

constexpr int kChunkWindows = 262144;

dvh::Opts make_opts(const dvh_options& p) {
  dvh::Opts o;
  o.eps = p.eps;
  o.eps_obj = p.eps_obj;
  o.step_safety = p.step_safety;
  o.rho = p.reflection;
  o.b_suff = p.restart_sufficient;
  o.b_nec = p.restart_necessary;
  o.b_art = p.restart_artificial;
  o.theta = p.primal_weight_theta;
  o.max_iters = p.max_iters;
  // a limit below the check period shortens the period (as the grid-wide path always did, dvh_large.hip): every tier
  // then runs a check at the limit, so an ITER_LIMIT window returns a checked candidate and its KKT numbers -- not
  // the NaN of "no check ran" and whatever the candidate images held (include/dervet_hip.h dvh_result)
  o.check_every = std::max(1, std::min(p.check_every, p.max_iters));
  o.kkt_every = p.kkt_every;
  o.ruiz_iters = p.ruiz_iters;
  o.power_iters = p.power_iters;
  o.warm = p.warm_start != 0;
  o.kkt_predict = p.kkt_predict;
  o.small_max = dvh::kSmallMax;
  return o;
}

dvh::Batch make_batch(const dvh_packed& bt) {
  return dvh::Batch{bt.desc, bt.indptr, bt.indices, bt.data, bt.c, bt.c0, bt.q, bt.l, bt.u,
                    bt.x, bt.y, bt.stats, bt.istats};
}

// The certificate pass over the batch (dvh_certify.hip), one launch on the solve's stream: after a solve (gate) its
// workgroups leave at once unless their window came back ITER_LIMIT or NUMERICAL -- the device-side gating of the
// interconnection form -- so the pass adds no host wait; the counters travel to a pinned host word behind it and are
// read after the solve's final wait (finish_timing).
int certify_pass(dvh_handle* h, const dvh_packed* bt, const std::vector<int64_t>& desc, int gate, hipStream_t s) {
  const int count = bt->count;
  const int64_t bn = desc[6], bm = desc[7], bz = desc[5];
  int64_t sn = 0, sm = 0, snz = 0;
  int mn = 1, mm = 1;
  for (int k = 0; k < count; ++k) {
    const int64_t* d = &desc[8 * (size_t)k];
    sn = std::max(sn, d[6] + d[0] - bn);
    sm = std::max(sm, d[7] + d[1] - bm);
    snz = std::max(snz, d[5] + d[3] - bz);
    if (d[0] > dvh::kSmallMax || d[1] > dvh::kSmallMax) continue;
    mn = std::max<int>(mn, (int)d[0]);
    mm = std::max<int>(mm, (int)d[1]);
  }
  const size_t D = sizeof(double), I = sizeof(int32_t);
  DVH_HIP(h, h->c_tptr.ensure(I * (size_t)(sn + count)));
  DVH_HIP(h, h->c_tind.ensure(I * (size_t)snz));
  DVH_HIP(h, h->c_tval.ensure(D * (size_t)snz));
  DVH_HIP(h, h->c_tau.ensure(D * (size_t)sn));
  DVH_HIP(h, h->c_gx.ensure(D * (size_t)sn));
  DVH_HIP(h, h->c_sig.ensure(D * (size_t)sm));
  DVH_HIP(h, h->c_gy.ensure(D * (size_t)sm));
  DVH_HIP(h, h->c_counts.ensure(I * 5));
  DVH_HIP(h, h->cert_host.ensure(I * 7));
  for (DevEvent& e : h->cert_ev) DVH_HIP(h, e.ensure());
  dvh::CertWork cw{h->c_tptr.as<int32_t>(), h->c_tind.as<int32_t>(), h->c_tval.as<double>(), h->c_tau.as<double>(),
                   h->c_gx.as<double>(), h->c_sig.as<double>(), h->c_gy.as<double>(), h->c_counts.as<int32_t>(),
                   bn, bm, bz};
  const int cap = h->opts.certify_iters > 0 ? h->opts.certify_iters : dvh::kCertifyDefaultCap;
  DVH_HIP(h, hipMemsetAsync(h->c_counts.p, 0, I * 5, s));
  DVH_HIP(h, hipEventRecord(h->cert_ev[0], s));
  DVH_HIP(h, dvh::launch_certify(make_batch(*bt), cw, count, mn, mm, cap, gate, s));
  DVH_HIP(h, hipEventRecord(h->cert_ev[1], s));
  DVH_HIP(h, hipMemcpyAsync(h->cert_host.p, h->c_counts.p, I * 5, hipMemcpyDeviceToHost, s));
  // the in-kernel certificates' counters (certify = 2, after a solve) ride along: no wait of their own
  h->cert_early_pending = gate && early_counters(h);
  if (h->cert_early_pending)
    DVH_HIP(h, hipMemcpyAsync(h->cert_host.as<int32_t>() + 5, h->c_early.p, I * 2, hipMemcpyDeviceToHost, s));
  h->cert_pending = true;
  return DVH_OK;
}

void certify_reset(dvh_handle* h) {
  for (int32_t& v : h->st.cert) v = 0;
  h->st.cert_early[0] = h->st.cert_early[1] = 0;
  h->cert_early_pending = false;
  h->st.cert_ms = 0.0;
  h->cert_pending = false;
}

bool is_large(const int64_t* d) { return d[0] > dvh::kSmallMax || d[1] > dvh::kSmallMax; }

// One chunk of the batch: its extents in the packed arrays, its small windows' maxima (the on-chip kernels' LDS
// sizing) and its medium-tier candidates.
struct ChunkPlan {
  dvh::Chunk ch;
  int64_t sn, sm, snz;
  int mn, mm;
  int64_t mnz;
  int nsmall;
  int nj;  // small windows of battery shape with J != 1 demand periods (device_cascade: the band kernel's instantiation)
  std::vector<int32_t> med;
  int med_T = 0;
};
struct BatchPlan {
  std::vector<ChunkPlan> chunks;
  std::vector<int> large;             // the windows above the on-chip limits, medium candidates included
  int64_t wn = 0, wm = 0, wnz = 0;    // the workspace: the largest chunk extents
  int wc = 0;
};

// Chunking + workspace sizing.  Medium tier candidates (chain_on): battery-shaped sizes (n = 3T + J, m <= 2T + 1) up
// to kPMax segments of kChainB steps; the plan kernel verifies the pattern, anything else goes to the grid-wide path.
BatchPlan scan_chunks(const std::vector<int64_t>& desc, int count, bool chain_on) {
  auto is_medium = [&](const int64_t* d) {
    const int64_t T = d[2] - 1;
    return chain_on && T > dvh::kChainB && T <= (int64_t)dvh::kPMax * dvh::kChainB && d[0] >= 3 * T &&
           d[0] <= 3 * T + dvh::kChainJMax && d[1] <= 2 * T + 1;
  };
  BatchPlan p;
  for (int first = 0; first < count; first += kChunkWindows) {
    ChunkPlan c{};
    c.ch.first = first;
    c.ch.count = std::min(kChunkWindows, count - first);
    const int64_t* d0 = &desc[8 * (size_t)first];
    c.ch.base_n = d0[6];
    c.ch.base_m = d0[7];
    c.ch.base_nz = d0[5];
    for (int k = first; k < first + c.ch.count; ++k) {
      const int64_t* d = &desc[8 * (size_t)k];
      c.sn = std::max(c.sn, d[6] + d[0] - c.ch.base_n);
      c.sm = std::max(c.sm, d[7] + d[1] - c.ch.base_m);
      c.snz = std::max(c.snz, d[5] + d[3] - c.ch.base_nz);
      if (is_large(d)) {
        p.large.push_back(k);
        if (is_medium(d)) {
          c.med.push_back(k);
          c.med_T = std::max<int>(c.med_T, (int)d[2] - 1);
        }
        continue;
      }
      ++c.nsmall;
      // n = 3 T + J, T = m_eq - 1: J = 0, 2 .. kJMax are the battery windows the single-demand-period instantiation of
      // the band kernel must not get (every other J != 1 is no battery window: both instantiations refuse it alike)
      const int64_t J = d[0] - 3 * (d[2] - 1);
      if (J == 0 || (J >= 2 && J <= dvh::kBandJMax)) ++c.nj;
      c.mn = std::max<int>(c.mn, (int)d[0]);
      c.mm = std::max<int>(c.mm, (int)d[1]);
      c.mnz = std::max(c.mnz, d[3]);
    }
    p.wn = std::max(p.wn, c.sn);
    p.wm = std::max(p.wm, c.sm);
    p.wnz = std::max(p.wnz, c.snz);
    p.wc = std::max(p.wc, c.ch.count);
    p.chunks.push_back(c);
  }
  return p;
}

// The handle's workspace grown to the plan's largest chunk, and the kernels' view of it.
int make_work(dvh_handle* h, const BatchPlan& p, dvh::Work& w) {
  const int64_t wn = p.wn, wm = p.wm, wnz = p.wnz;
  const int wc = p.wc;
  const size_t D = sizeof(double), I = sizeof(int32_t);
  DVH_HIP(h, h->w_tptr.ensure(I * (wn + wc)));
  DVH_HIP(h, h->w_tind.ensure(I * wnz));
  DVH_HIP(h, h->w_tval.ensure(D * wnz));
  DVH_HIP(h, h->w_kval.ensure(D * wnz));
  DVH_HIP(h, h->w_rowof.ensure(I * wnz));
  DVH_HIP(h, h->w_perm.ensure(I * wnz));
  DVH_HIP(h, h->w_dr.ensure(D * wm));
  DVH_HIP(h, h->w_dc.ensure(D * wn));
  DVH_HIP(h, h->w_cs.ensure(D * wn));
  DVH_HIP(h, h->w_ls.ensure(D * wn));
  DVH_HIP(h, h->w_us.ensure(D * wn));
  DVH_HIP(h, h->w_qs.ensure(D * wm));
  DVH_HIP(h, h->w_vbuf.ensure(D * wn));
  DVH_HIP(h, h->w_wbuf.ensure(D * wm));
  DVH_HIP(h, h->w_tmpc.ensure(D * wn));
  DVH_HIP(h, h->w_tmpr.ensure(D * wm));
  DVH_HIP(h, h->w_longk.ensure(I * (size_t)wc * dvh::kLMax));
  DVH_HIP(h, h->w_longt.ensure(I * (size_t)wc * dvh::kLMax));
  DVH_HIP(h, h->w_scal.ensure(D * (size_t)wc * dvh::kScal));
  DVH_HIP(h, h->w_fc.ensure(sizeof(float) * wn));
  DVH_HIP(h, h->w_fr.ensure(sizeof(float) * wm));
  DVH_HIP(h, h->w_queue.ensure(sizeof(int32_t)));
  w = dvh::Work{h->w_tptr.as<int32_t>(), h->w_tind.as<int32_t>(), h->w_tval.as<double>(), h->w_kval.as<double>(),
                h->w_rowof.as<int32_t>(), h->w_perm.as<int32_t>(), h->w_dr.as<double>(), h->w_dc.as<double>(),
                h->w_cs.as<double>(), h->w_ls.as<double>(), h->w_us.as<double>(), h->w_qs.as<double>(),
                h->w_vbuf.as<double>(), h->w_wbuf.as<double>(), h->w_tmpc.as<double>(), h->w_tmpr.as<double>(),
                h->w_longk.as<int32_t>(), h->w_longt.as<int32_t>(), h->d_hinv.as<double>(), h->w_scal.as<double>(),
                h->w_fc.as<float>(), h->w_fr.as<float>(), h->w_queue.as<int32_t>(), h->band_slots};
  DVH_HIP(h, h->d_list.ensure(I * 5 * (size_t)wc));  // the cascade's five device lists (dvh_route.hip)
  DVH_HIP(h, h->d_route.ensure(I * 8 * 5));
  DVH_HIP(h, h->route_host.ensure(I * 8 * 5));
  return DVH_OK;
}

// The next set of per-chunk timing events of the handle's pool (grown on demand).
int next_chunk_events(dvh_handle* h, const DevEvent*& out) {
  if (h->st.chunk_used == h->chunk_events.size()) h->chunk_events.emplace_back();
  std::array<DevEvent, 3>& ce = h->chunk_events[h->st.chunk_used];
  for (DevEvent& e : ce) DVH_HIP(h, e.ensure());  // (a set whose creation failed half-way is completed here)
  ++h->st.chunk_used;
  out = ce.data();
  return DVH_OK;
}

// The A/B paths over one chunk's small windows (kernel path 1: generic only; 2, or reflection rho != 1 -- the fast
// kernels are specialised to rho = 1: ELL -> generic), their lists formed on the host: the ELL kernel over the chunk
// -> the generic CSR kernel over the windows it returned (status -1).  The band kernels run in the device cascade only.
int host_list_tiers(dvh_handle* h, const dvh::Batch& b, const dvh::Work& w, const ChunkPlan& c, const dvh::Opts& o,
                    bool fast, const std::vector<int64_t>& desc, hipStream_t s) {
  const size_t I = sizeof(int32_t);
  auto large_at = [&](int k) { return is_large(&desc[8 * (size_t)k]); };
  // ELL widths from the setup statistics (one small D2H per chunk)
  std::vector<double> scal((size_t)c.ch.count * dvh::kScal);
  DVH_HIP(h, hipMemcpyAsync(scal.data(), w.scal, sizeof(double) * scal.size(), hipMemcpyDeviceToHost, s));
  DVH_HIP(h, sync_stream(h, s));
  int wx = 0, wy = 0;
  for (int k = 0; k < c.ch.count; ++k) {
    const double* sc = &scal[(size_t)k * dvh::kScal];
    if (sc[6] != 0.0) continue;
    wy = std::max(wy, (int)sc[8]);
    wx = std::max(wx, (int)sc[9]);
  }
  int variant = -1;
  hipError_t e = hipErrorInvalidValue;
  if (fast) {
    int ev = -1;
    e = dvh::launch_pdhg_ell(b, w, c.ch, o, c.mn, c.mm, wx, wy, s, &ev, nullptr, 0);
    if (e == hipSuccess) variant = ev;
  }
  std::vector<int32_t> generic;
  if (e == hipSuccess) {
    std::vector<int32_t> ist(2 * (size_t)c.ch.count);
    DVH_HIP(h, hipMemcpyAsync(ist.data(), b.istats + 2 * (size_t)c.ch.first, I * ist.size(),
                              hipMemcpyDeviceToHost, s));
    DVH_HIP(h, sync_stream(h, s));
    int nl = 0;
    for (int k = 0; k < c.ch.count; ++k) {
      if (large_at(c.ch.first + k)) {
        ++nl;
        continue;
      }
      if (ist[2 * (size_t)k] == -1) generic.push_back(c.ch.first + k);
    }
    h->st.n_ell += c.ch.count - (int)generic.size() - nl;
  } else if (e == hipErrorInvalidValue) {  // the generic path, or no ELL instantiation covers the chunk's sizes
    (void)hipGetLastError();
    for (int k = 0; k < c.ch.count; ++k)
      if (!large_at(c.ch.first + k)) generic.push_back(c.ch.first + k);
  } else {
    return hip_fail(h, e, "launch_pdhg_ell");
  }
  if (!generic.empty()) {
    DVH_HIP(h, hipMemcpyAsync(h->d_list.p, generic.data(), I * generic.size(), hipMemcpyHostToDevice, s));
    DVH_HIP(h, dvh::launch_power(b, w, c.ch, o, h->d_list.as<int32_t>(), (int)generic.size(), s));
    int gv = -1;
    e = dvh::launch_pdhg(b, w, c.ch, o, c.mn, c.mm, c.mnz, s, &gv, h->d_list.as<int32_t>(), (int)generic.size(),
                         early_counters(h));
    if (e == hipErrorInvalidValue)
      return fail(h, DVH_ERR_UNSUPPORTED, "window too large for the on-chip PDHG kernels (n or m > 4096)");
    if (e != hipSuccess) return hip_fail(h, e, "launch_pdhg");
    h->st.n_generic += (int)generic.size();
    if (variant < 0) variant = gv;
    DVH_HIP(h, sync_stream(h, s));  // d_list is reused by the next chunk
  }
  h->last_variant = variant;
  return DVH_OK;
}

// Solve a packed device batch given a host copy of its descriptors: scan -> workspace -> per chunk, the tiers of its
// small windows (the device cascade; dvh_set_kernel_path 1 / 2: the host-list A/B paths) and the medium tier -> the
// large windows -> the certificate pass.
int solve_packed(dvh_handle* h, const dvh_packed* bt, const std::vector<int64_t>& desc, hipStream_t s) {
  const int count = bt->count;
  certify_reset(h);
  const dvh::Opts o = make_opts(h->opts);
  const dvh::Batch b = make_batch(*bt);
  const bool fast = h->kernel_path != 1 && o.rho == 1.0;
  const bool cascade = fast && (h->kernel_path == 0 || h->kernel_path >= 3);
  const bool chain_on = (h->kernel_path == 0 || h->kernel_path >= 3) && o.rho == 1.0 && o.max_iters + o.power_iters < (1 << 17);
  const BatchPlan plan = scan_chunks(desc, count, chain_on);
  dvh::Work w;
  if (int rc = make_work(h, plan, w)) return rc;
  h->st.reset();
  if (h->opts.certify >= 2) {  // the early exit's counters: the handle's, zeroed ahead of the kernels that feed them
    DVH_HIP(h, h->c_early.ensure(sizeof(int32_t) * 2));
    DVH_HIP(h, hipMemsetAsync(h->c_early.p, 0, sizeof(int32_t) * 2, s));
  }
  DVH_HIP(h, hipEventRecord(h->ev[0], s));
  // dvh_set_launch_order: consumed by this solve; applied when it covers the batch, which is one chunk of small windows
  const size_t I = sizeof(int32_t);
  const int32_t* order = nullptr;
  h->order_used.swap(h->order);
  h->order.clear();
  if (!h->order_used.empty() && (int)h->order_used.size() == count && plan.chunks.size() == 1 &&
      plan.chunks[0].nsmall == count) {
    DVH_HIP(h, h->d_order.ensure(I * count));
    DVH_HIP(h, hipMemcpyAsync(h->d_order.as<int32_t>(), h->order_used.data(), I * count, hipMemcpyHostToDevice, s));
    order = h->d_order.as<int32_t>();
  }
  std::vector<char> med_done(count, 0);  // solved (or reported infeasible) by the medium tier
  // dvh_set_kernel_path 7: the heat form holds windows above kSmallMax (T = 768: n = 5,380, m = 4,609), which no chunk
  // counts among its small windows.  Those of its size (by the descriptor) are listed per chunk and examined by the form
  // behind the chunk's tiers; what it refuses (status -2) stays with the grid-wide path below.  One status read-back
  // for the whole batch, only when such windows exist.
  std::vector<int> heat_first(plan.chunks.size() + 1, 0);
  h->heat_list.clear();
  if (cascade && h->kernel_path == 7) {
    for (size_t ci = 0; ci < plan.chunks.size(); ++ci) {
      const dvh::Chunk& ch = plan.chunks[ci].ch;
      for (int k = ch.first; k < ch.first + ch.count; ++k) {
        const int64_t* d = &desc[8 * (size_t)k];
        if (is_large(d) && dvh::band_heat_sized(d[0], d[1], d[2])) h->heat_list.push_back(k);
      }
      heat_first[ci + 1] = (int)h->heat_list.size();
    }
    if (!h->heat_list.empty()) {
      DVH_HIP(h, h->d_heat_list.ensure(I * h->heat_list.size()));
      DVH_HIP(h, hipMemcpyAsync(h->d_heat_list.p, h->heat_list.data(), I * h->heat_list.size(), hipMemcpyHostToDevice, s));
    }
  }
  int heat_variant = -1;
  for (size_t ci = 0; ci < plan.chunks.size(); ++ci) {
    const ChunkPlan& c = plan.chunks[ci];
    const int nheat = heat_first[ci + 1] - heat_first[ci];
    if (c.nsmall == 0 && c.med.empty() && nheat == 0) continue;
    const DevEvent* ce = nullptr;
    if (int rc = next_chunk_events(h, ce)) return rc;
    DVH_HIP(h, hipEventRecord(ce[0], s));
    // (the device cascade sets up only what the band kernel refuses, inside device_cascade)
    if (c.nsmall > 0 && !cascade) DVH_HIP(h, dvh::launch_setup(b, w, c.ch, o, c.mn, c.mm, s));
    DVH_HIP(h, hipEventRecord(ce[1], s));
    if (c.nsmall > 0)
      if (int rc = cascade ? dvh::device_cascade(h, b, w, c.ch, o, c.nsmall, c.nj, plan.wc, c.mn, c.mm, s, order)
                           : host_list_tiers(h, b, w, c, o, fast, desc, s))
        return rc;
    if (int rc = dvh::chain_pass(h, b, w, c.ch, o, c.med, c.med_T, desc, med_done, s)) return rc;
    if (nheat > 0)
      DVH_HIP(h, dvh::launch_pdhg_band_heat(b, w, c.ch, o, s, h->d_heat_list.as<int32_t>() + heat_first[ci], nheat,
                                            &heat_variant, false));
    DVH_HIP(h, hipEventRecord(ce[2], s));
  }
  if (!h->heat_list.empty()) {  // which of them the form took: the others go on to the grid-wide path
    std::vector<int32_t> ist(2 * (size_t)count);
    DVH_HIP(h, hipMemcpyAsync(ist.data(), b.istats, I * ist.size(), hipMemcpyDeviceToHost, s));
    DVH_HIP(h, sync_stream(h, s));
    int took = 0;
    for (int k : h->heat_list)
      if (ist[2 * (size_t)k] != -2) {  // (-2: the band kernels' "not mine")
        med_done[k] = 1;
        ++took;
      }
    h->st.n_band += took;
    if (took > 0 && (h->last_variant < 0 || took == count)) h->last_variant = heat_variant;
  }
  // windows above the on-chip limits that the medium tier did not take: one at a time, the whole GPU each
  for (int k : plan.large) {
    if (med_done[k]) continue;
    if (!h->large) h->large.reset(dvh::large_create());
    std::string msg;
    hipError_t e = dvh::large_solve(h->large.get(), b, k, &desc[8 * (size_t)k], o, h->d_hinv.as<double>(), s, &msg,
                                    &h->st.large_ms[0], &h->st.large_ms[1]);
    if (e != hipSuccess) return fail(h, DVH_ERR_HIP, "window " + std::to_string(k) + ": " + msg);
    ++h->st.n_large;
  }
  // the opt-in certificate pass, behind the last tier (off: nothing is launched or allocated)
  if (h->opts.certify != 0)
    if (int rc = certify_pass(h, bt, desc, 1, s)) return rc;
  DVH_HIP(h, hipEventRecord(h->ev[3], s));
  return DVH_OK;
}

// dvh_certify_batch on a packed batch: the pass alone, over every window
int certify_packed(dvh_handle* h, const dvh_packed* bt, const std::vector<int64_t>& desc, hipStream_t s) {
  certify_reset(h);
  h->st.reset();
  DVH_HIP(h, hipEventRecord(h->ev[0], s));
  if (int rc = certify_pass(h, bt, desc, 0, s)) return rc;
  DVH_HIP(h, hipEventRecord(h->ev[3], s));
  return DVH_OK;
}

int finish_timing(dvh_handle* h, hipStream_t s) {
  DVH_HIP(h, sync_stream(h, s));
  SolveStats& st = h->st;
  float t = 0;
  st.timing[0] = st.timing[1] = st.timing[2] = 0;
  if (hipEventElapsedTime(&t, h->ev[0], h->ev[3]) == hipSuccess) st.timing[0] = t;
  if (h->cert_pending) {  // the certificate pass's counters and time (copied behind it on the stream)
    for (int i = 0; i < 5; ++i) st.cert[i] = h->cert_host.as<int32_t>()[i];
    if (h->cert_early_pending)
      for (int i = 0; i < 2; ++i) st.cert_early[i] = h->cert_host.as<int32_t>()[5 + i];
    h->cert_early_pending = false;
    if (hipEventElapsedTime(&t, h->cert_ev[0], h->cert_ev[1]) == hipSuccess) st.cert_ms = t;
    h->cert_pending = false;
  }
  for (size_t i = 0; i < st.chunk_used; ++i) {
    const auto& ce = h->chunk_events[i];
    if (hipEventElapsedTime(&t, ce[0], ce[1]) == hipSuccess) st.timing[1] += t;
    if (hipEventElapsedTime(&t, ce[1], ce[2]) == hipSuccess) st.timing[2] += t;
  }
  st.timing[1] += st.large_ms[0];
  st.timing[2] += st.large_ms[1];
  return DVH_OK;
}

// Contiguous, cost-balanced ranges of the batch for the handle's devices (windows the on-chip kernels take cost one
// workgroup each; larger windows run grid-wide and cost in proportion to their nonzeros; dervet_hip/parallel.py
// window_cost / shard_weighted are the same rule for ranks).
std::vector<int> split_batch(const dvh_lp* lps, int32_t count, int parts) {
  std::vector<double> cum(count + 1, 0.0);
  for (int k = 0; k < count; ++k) {
    const dvh_lp& lp = lps[k];
    const bool big = lp.n > dvh::kSmallMax || lp.m_eq + lp.m_ineq > dvh::kSmallMax;
    cum[k + 1] = cum[k] + (big ? std::max(1.0, lp.nnz / 5208.0) : 1.0);
  }
  std::vector<int> b(parts + 1, count);
  b[0] = 0;
  for (int r = 1; r < parts; ++r) {
    const double target = cum[count] * r / parts;
    int k = b[r - 1];
    while (k < count && cum[k] + 0.5 * (cum[k + 1] - cum[k]) < target) ++k;
    b[r] = k;
  }
  return b;
}

// Host LPs on one device: validated, packed, moved to the device, solved (screen: the certificate pass alone) and
// copied back.
int solve_batch_one(dvh_handle* h, const dvh_lp* lps, int32_t count, dvh_result* out, bool screen = false) {
  DVH_HIP(h, hipSetDevice(h->device));
  std::vector<int64_t> desc(8 * (size_t)count);
  int64_t tn = 0, tm = 0, tz = 0, tr = 0;
  for (int k = 0; k < count; ++k) {
    std::string msg = dvh::validate_lp(lps[k], k);
    if (!msg.empty()) return fail(h, DVH_ERR_ARG, msg);
    const dvh_lp& lp = lps[k];
    const int m = lp.m_eq + lp.m_ineq;
    int64_t* d = &desc[8 * (size_t)k];
    d[0] = lp.n;
    d[1] = m;
    d[2] = lp.m_eq;
    d[3] = lp.nnz;
    d[4] = tr;
    d[5] = tz;
    d[6] = tn;
    d[7] = tm;
    tr += m + 1;
    tz += lp.nnz;
    tn += lp.n;
    tm += m;
  }
  std::vector<int32_t> indptr(tr), indices(tz);
  std::vector<double> data(tz), c(tn), l(tn), u(tn), q(tm), c0(count);
  for (int k = 0; k < count; ++k) {
    const dvh_lp& lp = lps[k];
    const int64_t* d = &desc[8 * (size_t)k];
    const int m = (int)d[1];
    std::memcpy(&indptr[d[4]], lp.indptr, sizeof(int32_t) * (m + 1));
    if (lp.nnz) {
      std::memcpy(&indices[d[5]], lp.indices, sizeof(int32_t) * lp.nnz);
      std::memcpy(&data[d[5]], lp.data, sizeof(double) * lp.nnz);
    }
    std::memcpy(&c[d[6]], lp.c, sizeof(double) * lp.n);
    std::memcpy(&l[d[6]], lp.l, sizeof(double) * lp.n);
    std::memcpy(&u[d[6]], lp.u, sizeof(double) * lp.n);
    if (m) std::memcpy(&q[d[7]], lp.q, sizeof(double) * m);
    c0[k] = lp.c0;
  }
  const size_t D = sizeof(double), I = sizeof(int32_t);
  DVH_HIP(h, h->d_desc.ensure(desc.size() * sizeof(int64_t)));
  DVH_HIP(h, h->d_indptr.ensure(I * tr));
  DVH_HIP(h, h->d_indices.ensure(I * std::max<int64_t>(tz, 1)));
  DVH_HIP(h, h->d_data.ensure(D * std::max<int64_t>(tz, 1)));
  DVH_HIP(h, h->d_c.ensure(D * tn));
  DVH_HIP(h, h->d_l.ensure(D * tn));
  DVH_HIP(h, h->d_u.ensure(D * tn));
  DVH_HIP(h, h->d_x.ensure(D * tn));
  DVH_HIP(h, h->d_q.ensure(D * std::max<int64_t>(tm, 1)));
  DVH_HIP(h, h->d_y.ensure(D * std::max<int64_t>(tm, 1)));
  DVH_HIP(h, h->d_c0.ensure(D * count));
  DVH_HIP(h, h->d_stats.ensure(D * 4 * count));
  DVH_HIP(h, h->d_istats.ensure(I * 2 * count));
  hipStream_t s = h->stream;
  DVH_HIP(h, hipMemcpyAsync(h->d_desc.p, desc.data(), desc.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemcpyAsync(h->d_indptr.p, indptr.data(), I * tr, hipMemcpyHostToDevice, s));
  if (tz) {
    DVH_HIP(h, hipMemcpyAsync(h->d_indices.p, indices.data(), I * tz, hipMemcpyHostToDevice, s));
    DVH_HIP(h, hipMemcpyAsync(h->d_data.p, data.data(), D * tz, hipMemcpyHostToDevice, s));
  }
  DVH_HIP(h, hipMemcpyAsync(h->d_c.p, c.data(), D * tn, hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemcpyAsync(h->d_l.p, l.data(), D * tn, hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemcpyAsync(h->d_u.p, u.data(), D * tn, hipMemcpyHostToDevice, s));
  if (tm) DVH_HIP(h, hipMemcpyAsync(h->d_q.p, q.data(), D * tm, hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemcpyAsync(h->d_c0.p, c0.data(), D * count, hipMemcpyHostToDevice, s));
  std::vector<double> x0, y0;
  if (h->opts.warm_start || screen) {  // starting points (the screen: what an undecided window keeps): the caller's x / y buffers (zero where absent)
    x0.assign(tn, 0.0);
    y0.assign(std::max<int64_t>(tm, 1), 0.0);
    for (int k = 0; k < count; ++k) {
      const int64_t* d = &desc[8 * (size_t)k];
      if (out[k].x) std::memcpy(&x0[d[6]], out[k].x, D * d[0]);
      if (out[k].y && d[1]) std::memcpy(&y0[d[7]], out[k].y, D * d[1]);
    }
    DVH_HIP(h, hipMemcpyAsync(h->d_x.p, x0.data(), D * tn, hipMemcpyHostToDevice, s));
    DVH_HIP(h, hipMemcpyAsync(h->d_y.p, y0.data(), D * y0.size(), hipMemcpyHostToDevice, s));
  }
  const dvh_packed bt{count, 0, tn, tm, tz, tr, h->d_desc.as<int64_t>(), h->d_indptr.as<int32_t>(),
                      h->d_indices.as<int32_t>(), h->d_data.as<double>(), h->d_c.as<double>(), h->d_c0.as<double>(),
                      h->d_q.as<double>(), h->d_l.as<double>(), h->d_u.as<double>(), h->d_x.as<double>(),
                      h->d_y.as<double>(), h->d_stats.as<double>(), h->d_istats.as<int32_t>()};
  h->n_syncs = 0;
  int rc = screen ? certify_packed(h, &bt, desc, s) : solve_packed(h, &bt, desc, s);
  if (rc != DVH_OK) return rc;
  std::vector<double> x(tn), y(tm), stats(4 * (size_t)count);
  std::vector<int32_t> ist(2 * (size_t)count);
  DVH_HIP(h, hipMemcpyAsync(x.data(), h->d_x.p, D * tn, hipMemcpyDeviceToHost, s));
  if (tm) DVH_HIP(h, hipMemcpyAsync(y.data(), h->d_y.p, D * tm, hipMemcpyDeviceToHost, s));
  DVH_HIP(h, hipMemcpyAsync(stats.data(), h->d_stats.p, D * 4 * count, hipMemcpyDeviceToHost, s));
  DVH_HIP(h, hipMemcpyAsync(ist.data(), h->d_istats.p, I * 2 * count, hipMemcpyDeviceToHost, s));
  rc = finish_timing(h, s);
  if (rc != DVH_OK) return rc;
  for (int k = 0; k < count; ++k) {
    const int64_t* d = &desc[8 * (size_t)k];
    dvh_result& r = out[k];
    if (r.x) std::memcpy(r.x, &x[d[6]], D * d[0]);
    if (r.y && d[1]) std::memcpy(r.y, &y[d[7]], D * d[1]);
    r.obj = stats[4 * k];
    r.primal_res_rel = stats[4 * k + 1];
    r.dual_res_rel = stats[4 * k + 2];
    r.gap_rel = stats[4 * k + 3];
    r.status = ist[2 * k];
    r.iters = ist[2 * k + 1];
  }
  return DVH_OK;
}

}  // namespace

extern "C" {

int dvh_solve_batch(dvh_handle* h, const dvh_lp* lps, int32_t count, dvh_result* out) {
  if (!h) return DVH_ERR_ARG;
  if (count < 0 || (count > 0 && (!lps || !out))) return fail(h, DVH_ERR_ARG, "null lps/out or negative count");
  if (count == 0) return DVH_OK;
  if (h->peers.empty()) return solve_batch_one(h, lps, count, out);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<dvh_handle*> hs = {h};
  hs.insert(hs.end(), h->peers.begin(), h->peers.end());
  const int P = (int)hs.size();
  const std::vector<int> b = split_batch(lps, count, P);
  std::vector<int> rc(P, DVH_OK);
  std::vector<std::thread> th;
  for (int i = 1; i < P; ++i)
    if (b[i + 1] > b[i]) th.emplace_back([&, i] { rc[i] = solve_batch_one(hs[i], lps + b[i], b[i + 1] - b[i], out + b[i]); });
  if (b[1] > b[0]) rc[0] = solve_batch_one(h, lps, b[1], out);
  for (auto& t : th) t.join();
  SolveStats total;
  for (int i = 0; i < P; ++i) {
    if (rc[i] != DVH_OK) {
      const std::string msg = hs[i]->err;  // copy first: hs[0] is h
      return fail(h, rc[i], "device " + std::to_string(hs[i]->device) + " (part " + std::to_string(i) + "): " + msg);
    }
    if (b[i + 1] > b[i]) total.add(hs[i]->st);
  }
  total.timing[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  h->st = total;
  return DVH_OK;
}

// The certificate pass alone over host LPs (a screen before a solve): every on-chip window comes back PRIMAL_INFEASIBLE
// (ray in y), DUAL_INFEASIBLE (ray in x) or DVH_UNDECIDED; x / y of a window are otherwise the caller's.  Runs on the
// handle's first device.
int dvh_certify_batch(dvh_handle* h, const dvh_lp* lps, int32_t count, dvh_result* out) {
  if (!h) return DVH_ERR_ARG;
  if (count < 0 || (count > 0 && (!lps || !out))) return fail(h, DVH_ERR_ARG, "null lps/out or negative count");
  if (count == 0) {
    certify_reset(h);
    return DVH_OK;
  }
  return solve_batch_one(h, lps, count, out, true);
}

int dvh_solve_packed_device(dvh_handle* h, const dvh_packed* bt, void* stream) {
  if (!h) return DVH_ERR_ARG;
  if (!bt || bt->count < 0) return fail(h, DVH_ERR_ARG, "null or negative batch");
  if (bt->count == 0) return DVH_OK;
  if (!bt->desc || !bt->indptr || !bt->c || !bt->c0 || !bt->l || !bt->u || !bt->x || !bt->stats || !bt->istats)
    return fail(h, DVH_ERR_ARG, "null device array in packed batch");
  DVH_HIP(h, hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  h->n_syncs = 0;
  std::vector<int64_t> desc(8 * (size_t)bt->count);
  DVH_HIP(h, hipMemcpyAsync(desc.data(), bt->desc, desc.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  DVH_HIP(h, sync_stream(h, s));
  // host-side sanity of the descriptors (no device data is read beyond desc)
  for (int k = 0; k < bt->count; ++k) {
    const int64_t* d = &desc[8 * (size_t)k];
    if (d[0] <= 0 || d[1] < 0 || d[2] < 0 || d[2] > d[1] || d[3] < 0 || d[4] < 0 || d[5] < 0 || d[6] < 0 || d[7] < 0 ||
        d[4] + d[1] + 1 > bt->total_rows || d[5] + d[3] > bt->total_nnz || d[6] + d[0] > bt->total_n ||
        d[7] + d[1] > bt->total_m)
      return fail(h, DVH_ERR_ARG, "packed descriptor " + std::to_string(k) + " out of range");
    if (k > 0) {
      const int64_t* p = &desc[8 * (size_t)(k - 1)];
      if (d[5] < p[5] || d[6] < p[6] || d[7] < p[7])
        return fail(h, DVH_ERR_ARG, "packed descriptors must have non-decreasing offsets");
    }
  }
  int rc = solve_packed(h, bt, desc, s);
  if (rc != DVH_OK) return rc;
  return finish_timing(h, s);
}

}  // extern "C"
