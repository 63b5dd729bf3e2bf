// dvh_cascade.cpp -- the two tier drivers of one chunk of a solve (solve_packed, dvh_solve.cpp): the device cascade
// over its small windows and the medium tier over its battery-shaped large ones.
#include <cstdio>
#include <cstdlib>

#include "dvh_handle.h"

namespace dvh {

// Medium tier over the candidates of one chunk: plan (structure, segmentation, crossed bounds) -> setup of the
// planned windows (the one-workgroup setup kernel, or grid-wide for n >= kMedSetupNMax) -> team launches: windows of
// up to kChainMedMax segments together, longer ones (the 5-minute annual window) in launches of their own.
// med_done[k] = 1 for the windows solved or reported infeasible; the others stay with the grid-wide path, and so do
// the windows a launch had not finished when it aborted (a segment exchange outlasted the spin limit).
int chain_pass(dvh_handle* h, const dvh::Batch& b, const dvh::Work& w, const dvh::Chunk& ch, const dvh::Opts& o,
               const std::vector<int32_t>& med, int max_T, const std::vector<int64_t>& desc,
               std::vector<char>& med_done, hipStream_t s) {
  const int nm = (int)med.size();
  if (nm == 0) return DVH_OK;
  const size_t I = sizeof(int32_t);
  DVH_HIP(h, h->m_list.ensure(I * (size_t)nm));
  DVH_HIP(h, hipMemcpyAsync(h->m_list.p, med.data(), I * nm, hipMemcpyHostToDevice, s));
  DVH_HIP(h, h->m_plan.ensure(I * (size_t)nm * dvh::kPlanInts));
  hipError_t e = dvh::launch_chain_plan(b, w, ch, h->m_list.as<int32_t>(), nm, max_T, h->m_plan.as<int32_t>(), s);
  if (e != hipSuccess) return hip_fail(h, e, "launch_chain_plan");
  std::vector<int32_t> head((size_t)nm * 4);  // {P, T, J, k} of every plan record
  DVH_HIP(h, hipMemcpy2DAsync(head.data(), 4 * I, h->m_plan.p, I * dvh::kPlanInts, 4 * I, nm, hipMemcpyDeviceToHost, s));
  DVH_HIP(h, sync_stream(h, s));
  std::vector<int32_t> small_setup, accepted;
  for (int i = 0; i < nm; ++i) {
    const int P = head[4 * (size_t)i];
    if (P < 0) med_done[med[i]] = 1;  // crossed bounds: PRIMAL_INFEASIBLE from the plan kernel
    if (P <= 0) continue;
    accepted.push_back(i);
    if (desc[8 * (size_t)med[i]] < dvh::kMedSetupNMax) small_setup.push_back(med[i]);
  }
  if (accepted.empty()) return DVH_OK;
  // setup of the planned windows
  if (!small_setup.empty()) {
    int mn = 0;
    for (int k : small_setup) mn = std::max<int>(mn, (int)desc[8 * (size_t)k]);
    DVH_HIP(h, h->m_pos.ensure(I * small_setup.size()));
    DVH_HIP(h, hipMemcpyAsync(h->m_pos.p, small_setup.data(), I * small_setup.size(), hipMemcpyHostToDevice, s));
    e = dvh::launch_setup_medium(b, w, ch, o, mn, h->m_pos.as<int32_t>(), (int)small_setup.size(), s);
    if (e != hipSuccess) return hip_fail(h, e, "launch_setup_medium");
  }
  for (int i : accepted) {
    const int k = med[i];
    if (desc[8 * (size_t)k] < dvh::kMedSetupNMax) continue;
    e = dvh::launch_setup_long(b, w, ch, o, k, &desc[8 * (size_t)k], s);
    if (e != hipSuccess) return hip_fail(h, e, "launch_setup_long");
  }
  // the one-workgroup setup flags windows it cannot scale (more long rows than its lists): those go grid-wide
  std::vector<double> flag6(accepted.size(), 0.0);
  for (size_t a = 0; a < accepted.size(); ++a)
    DVH_HIP(h, hipMemcpyAsync(&flag6[a], w.scal + (int64_t)(med[accepted[a]] - ch.first) * dvh::kScal + 6,
                              sizeof(double), hipMemcpyDeviceToHost, s));
  DVH_HIP(h, sync_stream(h, s));
  std::vector<int32_t> groups[2];  // plan positions: [0] up to kChainMedMax segments, [1] longer
  int PTg[2] = {0, 0};
  for (size_t a = 0; a < accepted.size(); ++a) {
    if (flag6[a] != 0.0) continue;
    const int i = accepted[a], P = head[4 * (size_t)i];
    const int g = P > dvh::kChainMedMax ? 1 : 0;
    groups[g].push_back(i);
    PTg[g] = std::max(PTg[g], P);
  }
  if (h->chain_cap < 0) {
    int cap = 0;
    if (dvh::chain_capacity(h->device, &cap) != hipSuccess) cap = 0;
    (void)hipGetLastError();
    h->chain_cap = cap;
  }
  if (h->spin_ticks <= 0) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) khz = 100000;
    h->spin_ticks = (long long)khz * 1000 * 2;  // 2 s: a partner's hand-off normally takes microseconds
    // DVH_CHAIN_SPIN_TICKS (tests): another limit; < 0 aborts at the first exchange that has to wait, forcing the
    // abort -> grid-wide hand-over path
    if (const char* v = getenv("DVH_CHAIN_SPIN_TICKS")) {
      const long long t = atoll(v);
      if (t != 0) h->spin_ticks = t;
    }
  }
  const int S = h->chain_cap / 8;  // resident slots per XCD
  for (int g = 0; g < 2; ++g) {
    const int PT = PTg[g];
    if (groups[g].empty()) continue;
    const int NT = S >= 1 && PT <= 8 * S ? dvh::chain_team_count(S, PT) : 0;
    if (NT < 1) continue;  // cannot keep a team resident: the grid-wide path takes them
    constexpr int kMaxPerLaunch = 0x3FFF - 2;  // window tags keep 14 bits of a team's window count
    for (size_t a0 = 0; a0 < groups[g].size(); a0 += kMaxPerLaunch) {
      const int np = (int)std::min<size_t>(kMaxPerLaunch, groups[g].size() - a0);
      const int32_t* pos = groups[g].data() + a0;
      std::vector<int32_t> ks(np);
      for (int q = 0; q < np; ++q) ks[q] = med[pos[q]];
      DVH_HIP(h, h->m_pos.ensure(I * 2 * (size_t)np));
      int32_t* dpos = h->m_pos.as<int32_t>();
      DVH_HIP(h, hipMemcpyAsync(dpos, pos, I * np, hipMemcpyHostToDevice, s));
      DVH_HIP(h, hipMemcpyAsync(dpos + np, ks.data(), I * np, hipMemcpyHostToDevice, s));
      e = dvh::launch_chain_mark(b, dpos + np, np, s);
      if (e != hipSuccess) return hip_fail(h, e, "launch_chain_mark");
      DVH_HIP(h, h->m_xbuf.ensure(dvh::chain_xbuf_bytes(NT, PT)));
      DVH_HIP(h, h->m_abort.ensure(dvh::chain_abort_bytes(S)));
      e = dvh::launch_chain(b, w, ch, o, dpos, np, h->m_plan.as<int32_t>(), PT, S, h->m_xbuf.p,
                            h->m_abort.as<int32_t>(), h->spin_ticks, s);
      if (e == hipErrorCooperativeLaunchTooLarge) {  // not resident after all: leave them to the grid-wide path
        (void)hipGetLastError();
        h->chain_cap = 0;
        return DVH_OK;
      }
      if (e != hipSuccess) return hip_fail(h, e, "launch_chain");
      std::vector<int32_t> ab(dvh::chain_abort_bytes(S) / I);
      DVH_HIP(h, hipMemcpyAsync(ab.data(), h->m_abort.p, I * ab.size(), hipMemcpyDeviceToHost, s));
      DVH_HIP(h, sync_stream(h, s));
      if (getenv("DVH_CHAIN_PROBE_DUMP")) {  // timing probe builds: wave 0's waits per workgroup (wall-clock ticks)
        for (int gb = 0; gb < 8 * S; ++gb)
          if (ab[16 + 8 * (size_t)gb + 6] || ab[16 + 8 * (size_t)gb + 7])
            fprintf(stderr, "PROBE block %d tauwait %d hopwait %d\n", gb, ab[16 + 8 * (size_t)gb + 6],
                    ab[16 + 8 * (size_t)gb + 7]);
      }
      if (ab[0] != 0) {
        // a segment exchange outlasted the spin limit: the windows the launch finished keep their results, the
        // others (still marked pending) go to the grid-wide path; the diagnostics stay readable in dvh_last_error
        std::string msg = "medium tier: a segment exchange timed out (PT " + std::to_string(PT) + ", NT " +
                          std::to_string(NT) + "); unfinished windows moved to the grid-wide path; workgroups "
                          "{block: state list round entry tag seen}:";
        for (int gb = 0; gb < 8 * S; ++gb) {
          const int32_t* d = &ab[16 + 8 * (size_t)gb];
          if (d[0] == 0) continue;
          char buf[128];
          snprintf(buf, sizeof buf, " %d: %d %d %d 0x%x 0x%x 0x%x;", gb, d[0], d[1], d[2], d[3], d[4], d[5]);
          msg += buf;
        }
        h->st.warn += msg;
        ++h->st.n_chain_aborts;
        std::vector<int32_t> st(2);
        for (int q = 0; q < np; ++q) {
          DVH_HIP(h, hipMemcpy(st.data(), b.istats + 2 * (int64_t)ks[q], 2 * I, hipMemcpyDeviceToHost));
          if (st[0] != dvh::kChainPending) {
            med_done[ks[q]] = 1;
            ++h->st.n_chain;
          }
        }
        continue;
      }
      for (int q = 0; q < np; ++q) med_done[ks[q]] = 1;
      h->st.n_chain += np;
    }
  }
  return DVH_OK;
}

// The default kernel cascade over one chunk's small windows, its lists formed on the device (dvh_route.hip): the
// battery-banded kernel over the chunk -> its refusals (status -2) through the band-ICE form (both scale the windows
// they take themselves: no setup_kernel for them) -> what that refuses, set up (setup_kernel over the list), through
// the ELL kernels, in two size classes (the small market-day kernels' shapes, n <= 512 and m <= 768, and the
// rest), each instantiation sized for its class -> what they refuse (-1) or cannot hold through the generic CSR
// kernel, both classes in one launch.  With dvh_set_kernel_path 5 the band kernel's interconnection form (POI limit
// rows, curtailable PV, charge-from-PV rows) runs over the ICE pass's list right behind it; with 6 the load-shift form
// (controllable-load windows, dvh_band_shift.hip) does, in the same place; with 7 the heat form (windows with a
// combined-heat-and-power unit, dvh_band_heat.hip).
// One small read-back per stage that ran ({count, ELL widths, max n / m / nnz} of the windows it hands on; two after
// the ICE form when it refuses windows: their count, then their size classes once they are set up); a batch the band
// kernel takes whole waits once.
// nj: the chunk's battery-shaped windows with J != 1 demand periods, counted by the host from the descriptors it
// holds anyway (scan_chunks; the first band launch precedes every routing pass, so no device count could reach it
// without a wait of its own): 0 lets the three-step battery form run its single-demand-period instantiation, over the
// chunk and over any list taken from it; anything else keeps the generic instantiation for all of them.
int device_cascade(dvh_handle* h, const dvh::Batch& b, const dvh::Work& w, const dvh::Chunk& ch, const dvh::Opts& o,
                   int nsmall, int nj, int wc, int mn, int mm, hipStream_t s, const int32_t* order) {
  const size_t I = sizeof(int32_t);
  int32_t* L[5];
  for (int r = 0; r < 5; ++r) L[r] = h->d_list.as<int32_t>() + (size_t)r * wc;
  int32_t* info = h->d_route.as<int32_t>();  // 8 ints per route: {count, wx, wy, max n, max m, max nnz}
  int32_t* rh = h->route_host.as<int32_t>();
  if (h->cus <= 0 && hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess)
    h->cus = 256;
  // band kernel form: three steps per lane (two windows per CU) once the windows outnumber the CUs; a window alone
  // on its CU is faster in the one-step form (0.75 vs 0.97 us per iteration, profiles/r02x_band_forms.log)
  const int forced_form = h->kernel_path == 3 ? 1 : h->kernel_path == 4 ? 3 : 0;
  auto form_for = [&](int nl) { return forced_form ? forced_form : (nl <= h->cus ? 1 : 3); };
  // route: the windows of `in` (or the chunk) with status `want` and size class `cls` -> L[out], info slot `slot`
  auto route = [&](int slot, const int32_t* in, int n_in, int want, int cls, int out) -> hipError_t {
    return dvh::launch_route(b.desc, b.istats, w.scal, ch.first, n_in, in, want, dvh::kSmallMax, cls, 512, 768,
                             L[out], info + 8 * slot, s);
  };
  auto readback = [&](int slot0, int nslots) -> hipError_t {
    hipError_t e = hipMemcpyAsync(rh + 8 * slot0, info + 8 * slot0, 8 * I * nslots, hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : sync_stream(h, s);
  };
  const bool j1 = nj == 0;
  int variant = -1, bvar = -1;
  h->last_band_variant = -1;
  // the form's code without the instantiation's (dvh_last_stats reports one code per form, dvh_last_band_variant the
  // instantiation that ran)
  auto form_code = [](int v) { return v >= 0 && v % 100 >= dvh::kBandJ1 ? v - dvh::kBandJ1 : v; };
  // the battery forms iterate on [0, 1]-normalised boxes (dvh_band.hip BOX; bench 246.4k vs 239.7k windows/s,
  // profiles/r04m_ab_band_box.log); the few windows with an unbounded ch / dis / ene column (status -3) are re-run by
  // the plain form, which takes every one of them (same structure and scaling checks), after the same read-back.
  // The ICE form's box (elec / on too) is opt-in: it spills as much as the plain ICE form and ran 0.8 % slower on
  // config 5 (profiles/r04n_ab_ice_box.log).  DVH_BAND_BOX: 0 none, 1 (default) battery forms, 2 battery + ICE.
  const char* box_env = getenv("DVH_BAND_BOX");
  const int box_mode = box_env ? atoi(box_env) : 1;
  const bool box = box_mode >= 1, box_ice = box_mode >= 2;
  // (order: the chunk's windows in the caller's launch order, dvh_set_launch_order; the results do not depend on it)
  DVH_HIP(h, dvh::launch_pdhg_band(b, w, ch, o, s, false, form_for(ch.count), box, order, order ? ch.count : 0, j1, &bvar));
  DVH_HIP(h, route(0, nullptr, ch.count, -2, 0, 0));
  if (box) DVH_HIP(h, route(1, nullptr, ch.count, -3, 0, 1));
  DVH_HIP(h, readback(0, box ? 2 : 1));
  if (box && rh[8] > 0) {
    // the plain form over the windows without a box; it can refuse some of them itself (-2: factors outside float's
    // range, checked after scaling, which the box form never reached for them), so the -2 list is formed again, over
    // the chunk, once it has run -- one more read-back, only when such windows exist
    DVH_HIP(h, dvh::launch_pdhg_band(b, w, ch, o, s, false, form_for(rh[8]), false, L[1], rh[8], j1, nullptr));
    DVH_HIP(h, route(0, nullptr, ch.count, -2, 0, 0));
    DVH_HIP(h, readback(0, 1));
  }
  int cur = rh[0];
  h->st.n_band += nsmall - cur;
  if (nsmall - cur > 0) {
    variant = form_code(bvar);
    h->last_band_variant = bvar;
  }
  if (cur > 0) {  // pass 2: the band kernel's ICE form over pass 1's refusals
    DVH_HIP(h, dvh::launch_pdhg_band(b, w, ch, o, s, true, form_for(cur), box_ice, L[0], cur, false, &bvar));
    // dvh_set_kernel_path 5: the interconnection form (dvh_band_grid.hip) over the same list, behind the ICE form on
    // the stream: its workgroups leave at once unless their window is still refused (-2), so the route below sees the
    // final statuses and the mode adds no read-back.  (Which of the two forms took the pass's windows is not read
    // back either: the pass reports the interconnection form's variant code.)
    if (h->kernel_path == 5) DVH_HIP(h, dvh::launch_pdhg_band_grid(b, w, ch, o, s, L[0], cur, &bvar, early_counters(h)));
    // dvh_set_kernel_path 6: the load-shift form (dvh_band_shift.hip), launched the same way
    if (h->kernel_path == 6) DVH_HIP(h, dvh::launch_pdhg_band_shift(b, w, ch, o, s, L[0], cur, &bvar));
    // dvh_set_kernel_path 7: the heat form (dvh_band_heat.hip: windows with a combined-heat-and-power unit), likewise
    if (h->kernel_path == 7) DVH_HIP(h, dvh::launch_pdhg_band_heat(b, w, ch, o, s, L[0], cur, &bvar));
    DVH_HIP(h, route(1, L[0], cur, -2, 0, 4));
    if (box_ice) DVH_HIP(h, route(2, L[0], cur, -3, 0, 1));
    DVH_HIP(h, readback(1, box_ice ? 2 : 1));
    if (box_ice && rh[16] > 0) {  // the plain ICE form over the ICE windows without a box; its -2s listed again
      DVH_HIP(h, dvh::launch_pdhg_band(b, w, ch, o, s, true, form_for(rh[16]), false, L[1], rh[16], false, nullptr));
      DVH_HIP(h, route(1, L[0], cur, -2, 0, 4));
      DVH_HIP(h, readback(1, 1));
    }
    const int left = rh[8];
    h->st.n_band += cur - left;
    if (cur - left > 0 && variant < 0) variant = bvar;
    cur = left;
    if (cur > 0) {
      // what the band kernels refused, set up (the ELL / generic kernels and the ELL widths of the route statistics
      // read setup_kernel's outputs) and handed on by size class
      DVH_HIP(h, dvh::launch_setup(b, w, ch, o, mn, mm, s, L[4], cur));
      DVH_HIP(h, route(1, L[4], cur, -2, 1, 2));
      DVH_HIP(h, route(2, L[4], cur, -2, 2, 3));
      DVH_HIP(h, readback(1, 2));
    }
  }
  if (cur == 0) {
    h->last_variant = variant;
    return DVH_OK;
  }
  // ELL per size class (class c's windows in L[2 + c], info slot 1 + c; refusals -> L[c], the consumed lists)
  int ran[2] = {0, 0};
  for (int c = 0; c < 2; ++c) {
    const int32_t* in = rh + 8 * (1 + c);
    if (in[0] == 0) continue;
    int ev = -1;
    hipError_t e = dvh::launch_pdhg_ell(b, w, ch, o, in[3], in[4], in[1], in[2], s, &ev, L[2 + c], in[0],
                                        in[0] <= 2 * h->cus);
    if (e == hipSuccess) {
      if (variant < 0) variant = ev;
      DVH_HIP(h, route(3 + c, L[2 + c], in[0], -1, 0, c));
      ran[c] = 1;
    } else if (e == hipErrorInvalidValue) {  // no ELL instantiation holds this class: all generic
      (void)hipGetLastError();
    } else {
      return hip_fail(h, e, "launch_pdhg_ell");
    }
  }
  if (ran[0] || ran[1]) DVH_HIP(h, readback(3, 2));
  // the generic kernel over what is left of both classes, in one launch (one window per CU; a window's time does not
  // depend on the other windows', so the classes overlap inside the launch), sized for the windows it gets
  int gn = 0, gm[3] = {0, 0, 0};
  int32_t* gl = nullptr;
  for (int c = 0; c < 2; ++c) {
    const int32_t* in = rh + 8 * (1 + c);
    if (in[0] == 0) continue;
    const int32_t* g = ran[c] ? rh + 8 * (3 + c) : in;  // this class's windows for the generic kernel, their sizes
    int32_t* l = ran[c] ? L[c] : L[2 + c];
    if (ran[c]) h->st.n_ell += in[0] - g[0];
    if (g[0] == 0) continue;
    if (!gl) {
      gl = l;
    } else {  // append to the first class's list (disjoint subsets of the chunk: fits its wc slots)
      DVH_HIP(h, hipMemcpyAsync(gl + gn, l, I * g[0], hipMemcpyDeviceToDevice, s));
    }
    gn += g[0];
    for (int u = 0; u < 3; ++u) gm[u] = std::max(gm[u], (int)g[3 + u]);
  }
  if (gn > 0) {
    DVH_HIP(h, dvh::launch_power(b, w, ch, o, gl, gn, s));
    int gv = -1;
    hipError_t e = dvh::launch_pdhg(b, w, ch, o, gm[0], gm[1], gm[2], s, &gv, gl, gn, early_counters(h));
    if (e == hipErrorInvalidValue)
      return fail(h, DVH_ERR_UNSUPPORTED, "window too large for the on-chip PDHG kernels (n or m > 4096)");
    if (e != hipSuccess) return hip_fail(h, e, "launch_pdhg");
    h->st.n_generic += gn;
    if (variant < 0) variant = gv;
  }
  h->last_variant = variant;
  return DVH_OK;
}

}  // namespace dvh
