// dvh_handle.h -- the handle behind the C ABI and what the host units share of it (dvh_api*.cpp, dvh_solve.cpp,
// dvh_cascade.cpp).  Host only: no .hip file includes it; dvh_degradation.hip and dvh_sizing.cpp reach the handle
// through dvh::HandleView (dvh_internal.h), the latter so that the sanitizer driver can stand a stub in for it.
#pragma once
#include <array>
#include <string>

#include "dvh_host.h"

// Counters, diagnostics and timings of the last solve (the dvh_last_* getters copy out of it).
struct SolveStats {
  int n_ell = 0, n_generic = 0, n_large = 0, n_band = 0, n_chain = 0;
  int n_chain_aborts = 0;      // team launches that aborted (unfinished windows ran grid-wide); dvh_last_chain_aborts
  std::string warn;            // diagnostics of the solve's fallbacks (dvh_last_warning)
  float large_ms[2] = {0, 0};  // setup, PDHG time of the large windows
  size_t chunk_used = 0;       // the handle's chunk_events the solve recorded
  int32_t cert[5] = {0, 0, 0, 0, 0};  // certificate pass (dvh_last_certify), set by certify_reset / finish_timing
  int32_t cert_early[2] = {0, 0};     // in-kernel certificates (dvh_last_certify_early), set likewise
  double cert_ms = 0.0;
  double timing[3] = {0, 0, 0};  // whole solve, setup, PDHG (dvh_last_timing), set by finish_timing
  // a solve's start: everything it counts itself
  void reset() {
    n_ell = n_generic = n_large = n_band = n_chain = 0;
    n_chain_aborts = 0;
    warn.clear();
    large_ms[0] = large_ms[1] = 0.0f;
    chunk_used = 0;
  }
  // a device's part of a split batch: counts summed, the devices ran side by side so times take the longest
  void add(const SolveStats& p) {
    n_ell += p.n_ell;
    n_generic += p.n_generic;
    n_large += p.n_large;
    n_band += p.n_band;
    n_chain += p.n_chain;
    n_chain_aborts += p.n_chain_aborts;
    warn += p.warn;
    for (int u = 0; u < 4; ++u) cert[u] += p.cert[u];
    cert[4] = std::max(cert[4], p.cert[4]);
    cert_early[0] += p.cert_early[0];
    cert_early[1] = std::max(cert_early[1], p.cert_early[1]);
    cert_ms = std::max(cert_ms, p.cert_ms);
    for (int u = 1; u < 3; ++u) timing[u] = std::max(timing[u], p.timing[u]);
  }
};

// The stream, in a base of the handle so that it goes after every member.
struct dvh_handle_core {
  int device = 0;
  hipStream_t stream = nullptr;
  ~dvh_handle_core() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// The sizing state's owner.  A plain pointer inside, not a std::unique_ptr as large and comm are: dvh_sizing.cpp fills
// it through HandleView::sizing, a SizingState**, which the sanitizer driver's stand-in handle provides as well.
struct SizingSlot {
  dvh::SizingState* p = nullptr;
  SizingSlot() = default;
  SizingSlot(const SizingSlot&) = delete;
  SizingSlot& operator=(const SizingSlot&) = delete;
  ~SizingSlot() {
    if (p) dvh::sizing_destroy(p);
  }
};

// Everything a handle ever makes is a member that frees itself, so dvh_destroy (select the device, wait on the stream,
// delete) releases all of it.  Members go in reverse order of declaration: the pinned words (declared last), the
// device buffers, the events, large / comm / sizing, then the base's stream.
struct dvh_handle : dvh_handle_core {
  SizingSlot sizing;        // reliability sizing (dvh_sizing.cpp): device buffers, last call's timing
  dvh::CommOwner comm;      // dvh_comm_init: the result all-gather's RCCL communicator (dvh_comm.cpp)
  dvh::LargeOwner large;    // grid-wide path for windows above dvh::kSmallMax (created on first use)
  DevEvent ev[4];           // a solve's (an outage sweep's) first and last event: [0], [3]
  DevEvent cert_ev[2];      // the certificate pass's events
  // per-chunk timing events: a pool created on first use and reused by every solve (destroyed with the handle), so
  // no exit path of a solve can leak them; st.chunk_used = the events of the last solve
  std::vector<std::array<DevEvent, 3>> chunk_events;
  // scenario valuation (dvh_api_valuation.cpp): {bill, valuation} x {start, stop}, created by a call's first run
  DevEvent val_ev[2][2];
  bool val_ran[2] = {false, false};
  dvh_options opts{};
  std::string err;
  // packed inputs / outputs for the host API
  DevBuf d_desc, d_indptr, d_indices, d_data, d_c, d_c0, d_q, d_l, d_u, d_x, d_y, d_stats, d_istats;
  // workspace
  DevBuf w_queue;  // the band kernels' work-queue counter
  int band_slots[dvh::kPersistForms] = {};  // the persistent band forms' resident slots on this device (Work::slots)
  DevBuf w_tptr, w_tind, w_tval, w_kval, w_rowof, w_perm, w_dr, w_dc, w_cs, w_ls, w_us, w_qs, w_vbuf, w_wbuf,
      w_tmpc, w_tmpr, w_longk, w_longt, w_scal, w_fc, w_fr;
  DevBuf d_list, d_hinv;
  DevBuf m_list, m_plan, m_pos, m_xbuf, m_abort;  // medium tier (dvh_chain.hip)
  int chain_cap = -1;                             // resident 768-thread workgroups (cooperative limit)
  long long spin_ticks = 0;                       // chain kernel: longest exchange wait (wall-clock ticks)
  SolveStats st;
  DevBuf o_data, o_cases, o_len, o_hist, o_soe;  // reliability sweep
  DevBuf s_pairs, s_wts, s_bad;                   // seeded-sweep warm transfer (dvh_sweep.hip)
  DevBuf g_seeds, g_word;                         // scenario series generator (dvh_series.hip)
  DevBuf g_ev;                                    // device builder: the scanned EV step table (dvh_build_validate.h)
  DevBuf d_route;                                 // cascade lists' counts / ELL widths (dvh_route.hip)
  // certificate pass (dvh_certify.hip): its workspace (allocated on first use) and the device counters
  DevBuf c_tptr, c_tind, c_tval, c_tau, c_gx, c_sig, c_gy, c_counts;
  // certify = 2: {windows certified inside a PDHG kernel, their largest iteration count}, zeroed at a solve's start,
  // copied to cert_host[5 .. 6] behind the pass
  DevBuf c_early;
  bool cert_pending = false, cert_early_pending = false;
  DevBuf v_zwork;  // economic sizing's cut pass (dvh_api_value_sizing.cpp): z of the windows above the LDS size, G * T
  int n_syncs = 0;                                // host waits on the stream in the last solve
  double outage_ms = 0.0;
  int last_variant = -1;
  int last_band_variant = -1;  // the battery band pass's instantiation code (dvh_last_band_variant), -1: it took nothing
  int kernel_path = 0;  // 0 band -> ELL -> generic, 1 generic only, 2 ELL -> generic (no band kernel), 3 / 4 as 0
                        // with the battery band kernel's one-step / three-step form forced (0 picks by batch size),
                        // 5 as 0 plus the band kernel's interconnection form, 6 as 0 plus its load-shift form,
                        // 7 as 0 plus its heat form
  int cus = 0;          // compute units of the device (band kernel form choice)
  std::vector<int32_t> order;  // dvh_set_launch_order: the next solve's band-pass window order (empty: packing order)
  std::vector<int32_t> order_used;  // (the copy a solve consumed: kept until the next one, the H2D copy reads it)
  DevBuf d_order;
  // kernel path 7: the heat-sized windows above dvh::kSmallMax, which the heat form examines before the grid-wide path
  // (solve_packed); the host copy is kept until the next solve, the H2D copy reads it
  std::vector<int32_t> heat_list;
  DevBuf d_heat_list;
  // Further devices of this handle (device_mask bits after the first, or dvh_create_devices): same options; a
  // host-buffer batch is split into contiguous, cost-balanced ranges, one per device, solved concurrently (one host
  // thread per device, no inter-device traffic), results written straight into the caller's buffers.
  std::vector<dvh_handle*> peers;
  // pinned host mirrors: d_route's (one small read-back per tier) and c_counts' (copied behind the certificate pass,
  // read at the solve's final wait)
  PinnedBuf route_host, cert_host;
};

// Every host wait on a solve's stream goes through here (dvh_last_host_syncs reports the count of the last solve).
inline hipError_t sync_stream(dvh_handle* h, hipStream_t s) {
  ++h->n_syncs;
  return hipStreamSynchronize(s);
}

// The early-certificate counters for the kernels that test inside the loop, or null below level 2 (the launchers then
// take the instantiations without the test).
inline int32_t* early_counters(dvh_handle* h) { return h->opts.certify >= 2 ? h->c_early.as<int32_t>() : nullptr; }

inline int fail(dvh_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

inline int hip_fail(dvh_handle* h, hipError_t e, const char* where) {
  return fail(h, DVH_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

#define DVH_HIP(h, call)                                 \
  do {                                                   \
    hipError_t e_ = (call);                              \
    if (e_ != hipSuccess) return hip_fail(h, e_, #call); \
  } while (0)

namespace dvh {

// The tier drivers of one chunk (dvh_cascade.cpp), called by solve_packed (dvh_solve.cpp).
int device_cascade(dvh_handle* h, const Batch& b, const Work& w, const Chunk& ch, const Opts& o, int nsmall, int nj, int wc,
                   int mn, int mm, hipStream_t s, const int32_t* order);
int chain_pass(dvh_handle* h, const Batch& b, const Work& w, const Chunk& ch, const Opts& o,
               const std::vector<int32_t>& med, int max_T, const std::vector<int64_t>& desc,
               std::vector<char>& med_done, hipStream_t s);

}  // namespace dvh
