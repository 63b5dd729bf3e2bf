// dvh_api_build.cpp -- entry points that write a packed device batch or its inputs: the seeded-sweep warm transfer
// (dvh_sweep.hip), the scenario series generator (dvh_series.hip) and the device builder (dvh_build.hip).
#include <cmath>

#include "dvh_build_validate.h"
#include "dvh_handle.h"

extern "C" {

int dvh_warm_transfer_blend(dvh_handle* h, const dvh_packed* b, const int32_t* rows, const double* weights,
                            int32_t count, int32_t q) {
  if (!h) return DVH_ERR_ARG;
  if (q < 1 || q > dvh::kMaxBlend) return fail(h, DVH_ERR_ARG, "warm transfer: partners per window must be 1..8");
  if (count < 0 || (count > 0 && (!b || !rows || !weights))) return fail(h, DVH_ERR_ARG, "warm transfer: bad arguments");
  if (count == 0) return DVH_OK;
  if (!b->desc || !b->c || !b->u || !b->x || !b->y) return fail(h, DVH_ERR_ARG, "null device array in packed batch");
  const size_t R = (size_t)q + 2;
  // every window written once, no partner written (a workgroup would read it while another writes it), finite weights
  std::vector<char> target((size_t)std::max(b->count, 0), 0);
  for (int32_t i = 0; i < count; ++i) {
    const int32_t w = rows[R * i];
    if (w < 0 || w >= b->count)
      return fail(h, DVH_ERR_ARG, "warm transfer: row " + std::to_string(i) + " names no window");
    for (int32_t k = 0; k < q; ++k) {
      const int32_t p = rows[R * i + 1 + k];
      if (p < 0 || p >= b->count || w == p)
        return fail(h, DVH_ERR_ARG, "warm transfer: pair " + std::to_string(i) + " names no window / itself");
      if (!std::isfinite(weights[(size_t)q * i + k]))
        return fail(h, DVH_ERR_ARG, "warm transfer: weight of row " + std::to_string(i) + " is not finite");
    }
    if (target[w]) return fail(h, DVH_ERR_ARG, "warm transfer: window " + std::to_string(w) + " listed twice");
    target[w] = 1;
  }
  for (int32_t i = 0; i < count; ++i)
    for (int32_t k = 0; k < q; ++k)
      if (target[rows[R * i + 1 + k]])
        return fail(h, DVH_ERR_ARG, "warm transfer: partner of pair " + std::to_string(i) + " is itself a listed window");
  DVH_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  DVH_HIP(h, h->s_pairs.ensure(sizeof(int32_t) * R * (size_t)count));
  DVH_HIP(h, h->s_wts.ensure(sizeof(double) * (size_t)q * (size_t)count));
  DVH_HIP(h, h->s_bad.ensure(sizeof(int32_t)));
  DVH_HIP(h, hipMemcpyAsync(h->s_pairs.p, rows, sizeof(int32_t) * R * (size_t)count, hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemcpyAsync(h->s_wts.p, weights, sizeof(double) * (size_t)q * (size_t)count, hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemsetAsync(h->s_bad.p, 0, sizeof(int32_t), s));
  hipError_t e = dvh::launch_warm_transfer(b->desc, b->c, b->u, b->x, b->y, h->s_pairs.as<int32_t>(),
                                           h->s_wts.as<double>(), q, count, h->s_bad.as<int32_t>(), s);
  if (e != hipSuccess) return hip_fail(h, e, "launch_warm_transfer");
  int32_t bad = 0;
  DVH_HIP(h, hipMemcpyAsync(&bad, h->s_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  DVH_HIP(h, hipStreamSynchronize(s));
  if (bad) return fail(h, DVH_ERR_ARG, "warm transfer: " + std::to_string(bad) + " pair(s) of different LP shape");
  return DVH_OK;
}

int dvh_warm_transfer(dvh_handle* h, const dvh_packed* b, const int32_t* pairs, int32_t count) {
  if (!h) return DVH_ERR_ARG;
  if (count < 0 || (count > 0 && (!b || !pairs))) return fail(h, DVH_ERR_ARG, "warm transfer: bad arguments");
  const std::vector<double> ones((size_t)std::max(count, 0), 1.0);  // one partner, weight 1: the plain transfer
  return dvh_warm_transfer_blend(h, b, pairs, ones.data(), count, 1);
}

int dvh_series_draws(dvh_handle* h, const dvh_sweep_draws* d) {
  if (!h) return DVH_ERR_ARG;
  if (!d || d->count < 0 || d->steps < 1 || d->n_uniform < 0)
    return fail(h, DVH_ERR_ARG, "series draws: bad sizes");
  if (d->count == 0) return DVH_OK;
  if (!d->seeds || !d->z0 || !d->ar || (d->n_uniform > 0 && !d->uniform))
    return fail(h, DVH_ERR_ARG, "series draws: null array");
  DVH_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  DVH_HIP(h, h->g_seeds.ensure(sizeof(uint64_t) * (size_t)d->count));
  DVH_HIP(h, h->g_word.ensure(sizeof(int32_t)));
  DVH_HIP(h, hipMemcpyAsync(h->g_seeds.p, d->seeds, sizeof(uint64_t) * (size_t)d->count, hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemsetAsync(h->g_word.p, 0, sizeof(int32_t), s));
  hipError_t e = dvh::launch_series_draws(h->g_seeds.as<uint64_t>(), d->count, d->steps, d->n_uniform, d->a1,
                                          d->innov, d->z0, d->ar, d->uniform, h->g_word.as<int32_t>(), d->ambiguous,
                                          s);
  if (e != hipSuccess) return hip_fail(h, e, "launch_series_draws");
  int32_t amb = 0;
  DVH_HIP(h, hipMemcpyAsync(&amb, h->g_word.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  DVH_HIP(h, hipStreamSynchronize(s));
  if (amb && !d->ambiguous)
    return fail(h, DVH_ERR_UNSUPPORTED, "series draws: " + std::to_string(amb) +
                                            " scenario(s) met a ziggurat wedge test within 2^-40 of exp(); their "
                                            "draws may differ from numpy's");
  return DVH_OK;
}

int dvh_series_windows(dvh_handle* h, const dvh_window_series* w) {
  if (!h) return DVH_ERR_ARG;
  if (!w || w->G < 0 || w->T < 1 || w->t0 < 0 || w->rep < 1 || w->J < 0 || w->count < 1 || w->hours < 1 ||
      !(w->dt > 0.0) || (int64_t)(w->t0 + w->T - 1) / w->rep >= w->hours)
    return fail(h, DVH_ERR_ARG, "series windows: bad sizes (window past the series?)");
  if (w->G == 0) return DVH_OK;
  if (!w->rows || !w->ar || !w->site_load || !w->pv_profile || !w->price || !w->load_scale || !w->price_scale ||
      !w->pv_rated || !w->hp || !w->c0_add || !w->base || !w->retail || !w->c0)
    return fail(h, DVH_ERR_ARG, "series windows: null array");
  DVH_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  DVH_HIP(h, h->g_word.ensure(sizeof(int32_t)));
  DVH_HIP(h, hipMemsetAsync(h->g_word.p, 0, sizeof(int32_t), s));
  hipError_t e = dvh::launch_series_windows(*w, h->g_word.as<int32_t>(), s);
  if (e != hipSuccess) return hip_fail(h, e, "launch_series_windows");
  int32_t bad = 0;
  DVH_HIP(h, hipMemcpyAsync(&bad, h->g_word.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  DVH_HIP(h, hipStreamSynchronize(s));
  if (bad) return fail(h, DVH_ERR_ARG, "series windows: " + std::to_string(bad) + " row(s) outside 0 .. count - 1");
  return DVH_OK;
}

int dvh_build_battery_group(dvh_handle* h, const dvh_battery_group* g, const dvh_packed* b, int32_t first) {
  if (!h) return DVH_ERR_ARG;
  if (!g || !b) return fail(h, DVH_ERR_ARG, "null group or batch");
  if (g->G == 0) return DVH_OK;
  if (g->T < 1 || g->J < 0 || g->G < 0 || g->mI < 0 || !(g->dt > 0.0) || first < 0 || first + g->G > b->count)
    return fail(h, DVH_ERR_ARG, "battery group: bad sizes or window range");
  if ((g->mI > 0 && (!g->dcm_t || !g->dcm_j)) || !g->base || (g->J > 0 && !g->demand) || !g->E || !g->pch ||
      !g->pdis || !g->rte || !g->sdr || !g->soc_target || !g->ulsoc || !g->llsoc || !g->om || !g->c0 ||
      (g->has_retail && !g->retail) || (g->has_da && !g->da) || (g->has_emin && !g->emin) ||
      (g->has_emax && !g->emax) || (g->has_ice && (!g->ice_cap || !g->ice_pmin || !g->ice_cost)) ||
      (g->has_ev && (!g->ev_ch_max || !g->ev_target || !g->ev_code)))
    return fail(h, DVH_ERR_ARG, "battery group: null input array");
  if (g->has_ev && g->has_ice) return fail(h, DVH_ERR_ARG, "battery group: an EV is not combined with the ICE");
  // the EV's step codes (a host array) decide where its rows go: validated and scanned before anything is launched
  dvh::EvScan ev;
  if (g->has_ev) {
    const std::string msg = dvh::scan_ev_codes(g->ev_code, g->T, &ev);
    if (!msg.empty()) return fail(h, DVH_ERR_ARG, msg);
  }
  if (!b->desc || !b->indptr || !b->indices || !b->data || !b->c || !b->c0 || !b->q || !b->l || !b->u)
    return fail(h, DVH_ERR_ARG, "null device array in packed batch");
  DVH_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  // the windows' descriptors must describe exactly this LP shape, inside the arrays (the kernel writes through them)
  std::vector<int64_t> desc(8 * (size_t)g->G);
  DVH_HIP(h, hipMemcpyAsync(desc.data(), b->desc + 8 * (int64_t)first, desc.size() * sizeof(int64_t),
                            hipMemcpyDeviceToHost, s));
  // the demand-charge rows' steps and tau columns index the window's base series and columns: range-checked here
  // (an entry >= T or >= J made the kernel read base[] out of bounds and write column indices outside the
  // window), in the same sync as the descriptors
  std::vector<int32_t> dt_((size_t)g->mI), dj_((size_t)g->mI);
  if (g->mI > 0) {
    DVH_HIP(h, hipMemcpyAsync(dt_.data(), g->dcm_t, sizeof(int32_t) * dt_.size(), hipMemcpyDefault, s));
    DVH_HIP(h, hipMemcpyAsync(dj_.data(), g->dcm_j, sizeof(int32_t) * dj_.size(), hipMemcpyDefault, s));
  }
  if (g->has_ev) {  // (stream-ordered behind an earlier group's kernel, which reads the same buffer)
    DVH_HIP(h, h->g_ev.ensure(sizeof(int32_t) * ev.tab.size()));
    DVH_HIP(h, hipMemcpyAsync(h->g_ev.p, ev.tab.data(), sizeof(int32_t) * ev.tab.size(), hipMemcpyHostToDevice, s));
  }
  DVH_HIP(h, hipStreamSynchronize(s));
  for (int32_t i = 0; i < g->mI; ++i)
    if (dt_[i] < 0 || dt_[i] >= g->T || dj_[i] < 0 || dj_[i] >= g->J)
      return fail(h, DVH_ERR_ARG, "battery group: demand-charge row " + std::to_string(i) + " (step " +
                                      std::to_string(dt_[i]) + ", column " + std::to_string(dj_[i]) +
                                      ") outside T = " + std::to_string(g->T) + ", J = " + std::to_string(g->J));
  const bool ice = g->has_ice != 0, wide = ice || g->has_ev;
  const int64_t T = g->T, n = (wide ? 5 : 3) * T + g->J, meq = T + 1 + (g->has_ev ? T + ev.D : 0),
                m = meq + g->mI + (ice ? 2 * T : 0),
                nnz = 4 * T + (wide ? 4 : 3) * (int64_t)g->mI + (ice ? 4 * T : 0) + ev.nnz;
  for (int w = 0; w < g->G; ++w) {
    const int64_t* d = &desc[8 * (size_t)w];
    if (d[0] != n || d[1] != m || d[2] != meq || d[3] != nnz || d[4] < 0 || d[5] < 0 || d[6] < 0 || d[7] < 0 ||
        d[4] + m + 1 > b->total_rows || d[5] + nnz > b->total_nnz || d[6] + n > b->total_n || d[7] + m > b->total_m)
      return fail(h, DVH_ERR_ARG, "battery group: descriptor of window " + std::to_string(first + w) +
                                      " does not match the group's LP shape or the arrays");
  }
  const dvh::EvLayout lay{g->has_ev ? h->g_ev.as<int32_t>() : nullptr, ev.D, ev.nnz, ev.n_trail};
  hipError_t e = dvh::launch_build_battery(*g, lay, *b, first, s);
  if (e != hipSuccess) return hip_fail(h, e, "launch_build_battery");
  return DVH_OK;
}

}  // extern "C"
