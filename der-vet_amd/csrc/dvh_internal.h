// Internal declarations shared by the C-ABI layer (dvh_api*.cpp, dvh_solve.cpp, dvh_cascade.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>

struct dvh_window_series;  // include/dervet_hip.h
struct dvh_battery_group;
struct dvh_packed;
struct dvh_options;
struct dvh_handle;

namespace dvh {

constexpr int kWave = 64;
constexpr int kLongRow = 32;   // CSR rows longer than this are reduced by a whole wave
constexpr int kLMax = 64;      // long rows per matrix per window handled on chip
constexpr int kScal = 16;      // per-window scalars written by the setup kernel
constexpr int kHalpernTab = 65536;  // table of Halpern weights 1/(k+2)
constexpr int kSmallMax = 4096;     // windows with n or m above this go to the medium tier or the large-LP path
// Medium tier (dvh_chain.hip): battery windows of up to kPMax segments of kChainB steps, one workgroup per segment.
// Windows of up to kChainMedMax segments run as a batch (teams inside one XCD where they fit); longer ones (the
// 5-minute annual window of BASELINE config 3: T = 105,120, 137 segments) run in a launch of their own, one team
// spanning the chip.
constexpr int kChainB = 768;
constexpr int kPMax = 192;
constexpr int kChainMedMax = 16;
constexpr int kChainJMax = 256;     // tau (demand) columns per medium window
constexpr int kChainJSeg = 4;       // tau columns per segment
// plan words per window: [0] P, [1] T, [2] J, [3] k, [kPlanStart + s] first step of segment s (P + 1 entries),
// per (segment s, slot u): the tau column [kPlanSlot + 4 s + u] (-1: none) and the contiguous range of segments that
// share it [kPlanLo / kPlanHi + 4 s + u] (every segment of the range holds the column in a slot)
constexpr int kPlanStart = 4;
constexpr int kPlanSlot = kPlanStart + kPMax + 4;
constexpr int kPlanLo = kPlanSlot + kChainJSeg * kPMax;
constexpr int kPlanHi = kPlanLo + kChainJSeg * kPMax;
constexpr int kPlanInts = kPlanHi + kChainJSeg * kPMax;
// windows whose n reaches this are set up grid-wide (setup_long, dvh_chain.hip): the one-workgroup setup kernel keeps
// n + 1 transpose cursors in LDS
constexpr int kMedSetupNMax = 40000;

// A column's output value: the scaled x~ times its factor d, clipped to the caller's bounds.  The iterate is clipped
// to l / d and u / d, and (l / d) d can land one ulp outside [l, u]: the result contract promises l <= x <= u exactly
// (include/dervet_hip.h dvh_result, tests/result_contract.py), so every tier's write-back goes through here.  A NaN
// (a diverged window, status NUMERICAL) stays NaN: fmin / fmax alone would turn it into a bound.
__host__ __device__ inline double unscale_x(double xs, double d, double l, double u) {
  const double v = xs * d;
  return v != v ? v : fmin(fmax(v, l), u);
}

// Kernel-side copy of dvh_options (POD, passed by value).
struct Opts {
  double eps, step_safety, rho, b_suff, b_nec, b_art, theta;
  double eps_obj;      // objective-error termination (dvh_options.eps_obj; 0 = off)
  int max_iters, check_every, kkt_every, ruiz_iters, power_iters;
  int setup_segments;  // set by launch_setup
  int small_max;       // setup skips (scal[6] = 2) windows with n or m above this
  int warm;            // start from the (unscaled) x / y in the output buffers (band kernel; others cold)
  int kkt_predict;     // dvh_options.kkt_predict (band kernel; 0 = off)
};

// Inputs of one chunk of the packed batch (device pointers, global offsets from desc).
struct Batch {
  const int64_t* desc;
  const int32_t* indptr;
  const int32_t* indices;
  const double* data;
  const double* c;
  const double* c0;
  const double* q;
  const double* l;
  const double* u;
  double* x;
  double* y;
  double* stats;
  int32_t* istats;
};

// Per-chunk device workspace.  Window k of the chunk uses offsets (desc offsets - chunk base).
struct Work {
  int32_t* tptr;    // [sum(n+1)]   K^T row pointers        at (off_n - base_n) + (k - first)
  int32_t* tind;    // [sum nnz]    K^T column (= K row) ids
  double* tval;     // [sum nnz]    scaled K^T values
  double* kval;     // [sum nnz]    scaled K values
  int32_t* rowof;   // [sum nnz]    K entry -> row
  int32_t* perm;    // [sum nnz]    K entry -> K^T slot
  double* dr;       // [sum m]
  double* dc;       // [sum n]
  double* cs;       // [sum n]  Dc c
  double* ls;       // [sum n]  l / Dc
  double* us;       // [sum n]  u / Dc
  double* qs;       // [sum m]  Dr q
  double* vbuf;     // [sum n]
  double* wbuf;     // [sum m]
  double* tmpc;     // [sum n]
  double* tmpr;     // [sum m]
  int32_t* longk;   // [count * kLMax]  long rows of K
  int32_t* longt;   // [count * kLMax]  long rows of K^T (dense columns, e.g. the DCM tau)
  const double* hinv;  // [kHalpernTab] 1 / (k + 2), k = 0.. (Halpern anchor weights, exact IEEE quotients)
  double* scal;     // [count * kScal]  eta, w0, ||c||, ||q||, nlong(K), nlong(K^T), flag, ||K||,
                    //   max short row len K, K^T (<= 8), #rows > 8 in K, K^T
  float* fc;        // [sum n]  Dc rounded to single precision (the band kernel's KKT checks; written by the band
                    //          kernels, whose factors stay within [2^-100, 2^100])
  float* fr;        // [sum m]  Dr rounded to single precision
  int32_t* queue;   // [1] the band kernels' work-queue counter (zeroed before each launch)
  int* slots;       // HOST [kPersistForms]: resident workgroup slots of each persistent band form on this handle's
                    //   device (0: not measured yet); per handle, so that handles of a multi-device handle, driven
                    //   by their own host threads, never share it
};
constexpr int kPersistForms = 12;  // (ICE, GATE, BOX) of the persistent band kernels, then (GATE, BOX) of the J1 ones

struct Chunk {
  int first;        // first window index (global)
  int count;
  int64_t base_n, base_m, base_nz;
};

// Launchers (dvh_kernels.hip).  Return hipError_t.
// list (nlist entries): global window indices, or null for the whole chunk.
hipError_t launch_setup(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, int max_n, int max_m,
                        hipStream_t s, const int32_t* list = nullptr, int nlist = 0);
// Solve kernel selection is made from the chunk maxima; returns hipErrorInvalidValue when no
// instantiation covers the sizes (the caller reports DVH_ERR_UNSUPPORTED).
// Generic (CSR) kernel; list = optional device list of window ids (nlist blocks) instead of the whole chunk.
// early (device, int32[2]; dvh_options.certify = 2) != null: the instantiations with the in-kernel Farkas test (the
// certificate block below); early[0] += the windows they certify, early[1] = max(early[1], their iteration counts).
hipError_t launch_pdhg(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, int max_n, int max_m,
                       int64_t max_nnz, hipStream_t s, int* variant_out, const int32_t* list, int nlist,
                       int32_t* early = nullptr);
// ELL fast-path kernel over the whole chunk, or over the listed windows (wx, wy: ELL widths for K^T and K).
// Windows that do not fit its shape come back with istats status -1 (kNeedsGeneric) and must be re-run by
// launch_pdhg.
// latency: a list of at most two windows per CU (small variants only where they beat the 512-thread kernels).
hipError_t launch_pdhg_ell(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, int max_n, int max_m,
                           int wx, int wy, hipStream_t s, int* variant_out, const int32_t* list, int nlist,
                           bool latency = false);
// Battery-banded kernel (dvh_band.hip) over the whole chunk.  Windows whose CSR is not the battery + DCM
// window shape come back with istats status -2 (kNeedsEll) and must be re-run by launch_pdhg_ell.
// ice: the variant with LP-relaxed ICE columns (elec, on) and rows; list (nlist entries): global window indices,
// or null for the whole chunk; form: steps per lane of the battery kernel (3 default, 1 = the 768-thread form);
// variant_out: 9000000 + 1000 (steps per lane - 1) + 100 ice + waves per window (+ kBandJ1: the three-step form's
// single-demand-period instantiation).
// j1: no window of the list (or chunk) is a battery window with J != 1 demand periods, so the persistent three-step
// form may take its single-demand-period instantiation (J a compile-time 1); the other forms ignore it.
// box (battery forms): iterate on the columns' [0, 1]-normalised boxes (dvh_band.hip, BOX); windows with an unbounded
// ch / dis / ene column come back with status -3 (kNeedsPlain) and must be re-run with box = false.
hipError_t launch_pdhg_band(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s, bool ice,
                            int form, bool box, const int32_t* list, int nlist, bool j1, int* variant_out);
constexpr int kBandJ1 = 50;
constexpr int kBandJMax = 4;  // tau (demand-period) columns per band window
// Its persistent forms (dvh_band_persist.hip), the default for the three-step battery form and the ICE form unless
// DVH_BAND_QUEUE=0 (DVH_BAND_QUEUE_ICE=0: the ICE form only); gate: dvh_options.kkt_predict > 0.
hipError_t launch_band_persist(bool gate, bool box, bool j1, const Batch& b, const Work& w, const Chunk& ch,
                               const Opts& o, hipStream_t s, const int32_t* list, int nlist, int* variant_out);
hipError_t launch_band_persist_ice(bool gate, bool box, const Batch& b, const Work& w, const Chunk& ch, const Opts& o,
                                   hipStream_t s, const int32_t* list, int nlist, int* variant_out);
size_t setup_lds_bytes(int max_n, int max_m);
// Setup (scaling, transpose) of the listed medium windows (scaling vectors kept in the global workspace).
hipError_t launch_setup_medium(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, int max_n,
                               const int32_t* list, int nlist, hipStream_t s);
// Medium tier (dvh_chain.hip): plan (structure check + segmentation, plan[kPlanInts] per listed window, plan[0] =
// P, 0 = not this tier, -1 = reported infeasible by the setup) and the team kernel over the windows at positions
// pos[] of the plan (PT workgroups per team, NT teams, cooperative launch; xbuf >= chain_xbuf_bytes(NT, PT)).
// The plan reads only the window's own (unscaled) data: it runs before the setup, reports crossed bounds itself
// (PRIMAL_INFEASIBLE, plan[0] = -1) and leaves the step -> DCM row / tau maps in the window's vbuf workspace.
hipError_t launch_chain_plan(const Batch& b, const Work& w, const Chunk& ch, const int32_t* list, int nlist,
                             int max_T, int32_t* plan, hipStream_t s);
// Grid-wide setup (scaling, scaled data, norms: what setup_kernel writes for the chain kernel) of one planned window
// whose n is too large for the one-workgroup setup; uses the plan's maps.
hipError_t launch_setup_long(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, int k, const int64_t* d,
                             hipStream_t s);
// istats status of the listed windows set to kChainPending before a team launch: after an aborted launch the windows
// still pending go to the grid-wide path
constexpr int kChainPending = -7;
hipError_t launch_chain_mark(const Batch& b, const int32_t* list, int nlist, hipStream_t s);
hipError_t chain_capacity(int device, int* blocks);
size_t chain_xbuf_bytes(int NT, int PT);
size_t chain_abort_bytes(int S);  // abort word, window counter, per-workgroup diagnostics (grid 8 S)
// S: resident workgroup slots per XCD (grid = 8 S); teams of PT workgroups, chain_team_count(S, PT) of them
int chain_team_count(int S, int PT);
// spin_ticks: the longest a segment waits for a partner's exchange (wall-clock ticks) before the launch aborts
hipError_t launch_chain(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, const int32_t* pos, int npos,
                        const int32_t* plan, int PT, int S, void* xbuf, int32_t* abort_word, long long spin_ticks,
                        hipStream_t s);
// Seeded-sweep warm starts (dvh_sweep.hip): rows[count][q + 2] = {window, partner windows (q), T (> 0: battery + DCM
// dual scaling)}, wts[count][q] the partners' weights; bad counts rows whose windows differ in shape (skipped).
constexpr int kMaxBlend = 8;  // partners per window
hipError_t launch_warm_transfer(const int64_t* desc, const double* c, const double* u, double* x, double* y,
                                const int32_t* rows, const double* wts, int q, int count, int32_t* bad, hipStream_t s);
// Synthetic scenario series (dvh_series.hip): numpy-identical draws, one thread per scenario (ambiguous counts
// scenarios with a wedge test too close to call), and the device builder's inputs of G windows (bad counts rows out of
// range).
hipError_t launch_series_draws(const uint64_t* seeds, int count, int steps, int n_unif, double a1, double innov,
                               double* z0, double* ar, double* unif, int32_t* ambiguous, int32_t* amb_rows,
                               hipStream_t s);
hipError_t launch_series_windows(const ::dvh_window_series& w, int32_t* bad, hipStream_t s);
// Device builder (dvh_build.hip): windows first .. first + g.G - 1 of the packed batch written from the group's series.
// tab: device [3T] of a group with has_ev (dvh_build_validate.h EvScan), else unused
struct EvLayout {
  const int32_t* tab;
  int32_t D, nnz, n_trail;
};
hipError_t launch_build_battery(const ::dvh_battery_group& g, const EvLayout& ev, const ::dvh_packed& b, int first,
                                hipStream_t s);
// Cascade lists on the device (dvh_route.hip): the small windows of [first, first + count) -- or of in_list[0 ..
// count) -- whose status is `want` (cls 1: and n <= lim_n, m <= lim_m; cls 2: the others; cls 0: any size), in order,
// to out_list; out_info[0..5] = {their number, max ELL widths wx, wy, max n, m, nnz} over them.
hipError_t launch_route(const int64_t* desc, const int32_t* istats, const double* scal, int first, int count,
                        const int32_t* in_list, int want, int small_max, int cls, int lim_n, int lim_m,
                        int32_t* out_list, int32_t* out_info, hipStream_t s);
// Power iteration for ||Kt||_2 of the listed windows (generic path; the ELL kernel does its own on chip).
hipError_t launch_power(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, const int32_t* list, int nlist,
                        hipStream_t s);

// Post-facto reliability sweep (dvh_outage.hip): one case of dvh_outage_case with device pointers.
struct OutageCase {
  int n_steps, max_steps, outage_len, pad;
  int64_t len_off, hist_off;  // offsets into the lengths / histogram outputs
  double dt, soe0, dg_gen, gamma, soe_min, soe_max, charge_max, discharge_max, rte;
  const double *critical_load, *pv_max, *pv_vari, *init_soe, *load_shed;
};
// One thread per (case, start step); hist must be zeroed (sum of outage_len + 1 bins); lengths may be null.
hipError_t launch_outage(const OutageCase* d_cases, int ncase, int max_steps_n, int max_bins, int32_t* d_lengths,
                         int32_t* d_hist, hipStream_t s);
// min_soe_iterative mode: soe_used (max - min SOE of a target-length outage from soe0) per start.
hipError_t launch_outage_min_soe(const OutageCase* d_cases, int ncase, int max_steps_n, double* d_soe_used,
                                 hipStream_t s);

// The sizing loop's scan: d_first[case] (preset to INT32_MAX) <- the smallest uncovered start, d_count[case] (preset
// to 0) += the number of uncovered starts, of an outage_len-step outage from soe0 at every start.
hipError_t launch_outage_first_uncovered(const OutageCase* d_cases, int ncase, int max_steps_n, int32_t* d_first,
                                         int32_t* d_count, hipStream_t s);

// Reliability sizing LP on the device (dvh_sizing.hip; include/dervet_hip.h dvh_sizing_windows): one LP of the packed
// batch per entry, window `b` of the batch = entry b.  Device pointers; starts[K] are steps of the series.
struct SizingLP {
  const double *cl, *pv_vari, *shed;  // [n_steps] critical load, [n_steps] PV x nu or null, [>= L] % kept or null
  int32_t* starts;                    // [>= K] outage starts; new_start >= 0 is stored at starts[K - 1] first
  int n_steps, K, L, new_start;
  double dt, dg_gen, rte, llsoc, ulsoc, a0;  // a0 = min(soc_init, ulsoc)
  double lE, uE, lP, uP, cE, cP, c0;
};
// Expands nlp LPs into the packed arrays through their descriptors (desc[8 b ..], shapes n = 2 + 3 K L, m = 6 K L,
// m_eq = K L, nnz = 14 K L, checked by the caller).
hipError_t launch_build_sizing(const SizingLP* d_lps, int nlp, const int64_t* desc, int32_t* indptr, int32_t* indices,
                               double* data, double* c, double* c0, double* q, double* l, double* u, hipStream_t s);
// sizes[4 b .. 4 b + 3] = {x[off_n], x[off_n + 1], status, iterations} of window b (the E and P columns).
hipError_t launch_gather_sizes(const int64_t* desc, const double* x, const int32_t* istats, int nlp, double* sizes,
                               hipStream_t s);

// The handle's opaque sub-objects, each defined and destroyed by its own unit: the handle holds them as owners.
struct SizingState;  // reliability sizing (dvh_sizing.cpp)
void sizing_destroy(SizingState* s);
struct LargeSolver;  // grid-wide PDHG for one window too large for the workgroup-per-window kernels (dvh_large.hip)
LargeSolver* large_create();
void large_destroy(LargeSolver* ls);
struct Comm;  // the result all-gather's RCCL communicator (dvh_comm.cpp)
void comm_destroy(Comm* c);
template <auto Destroy>
struct DestroyWith {
  template <class T>
  void operator()(T* p) const { Destroy(p); }
};
using LargeOwner = std::unique_ptr<LargeSolver, DestroyWith<large_destroy>>;
using CommOwner = std::unique_ptr<Comm, DestroyWith<comm_destroy>>;

// What dvh_sizing.cpp and dvh_degradation.hip need of a handle (the other host units include dvh_handle.h;
// handle_view is in dvh_api.cpp, and the sizing sanitizer driver has a stand-in).
struct HandleView {
  int device;
  hipStream_t stream;
  dvh_options* opts;
  std::string* err;
  SizingState** sizing;  // the handle's (freed by sizing_destroy with it), created by the first sizing call
};
HandleView handle_view(dvh_handle* h);
inline int fail(const HandleView& v, int code, const std::string& msg) {
  *v.err = msg;
  return code;
}
#define DVH_VIEW_HIP(v, call)                                                                                  \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess) return dvh::fail(v, DVH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)


// The communicator's calls (dvh_comm_init / dvh_gather_results).  Return codes are the DVH_* codes; messages go to *err.
constexpr int kCommIdBytes = 128;  // ncclUniqueId
int comm_unique_id(unsigned char* id, std::string* err);
int comm_init(int device, int rank, int world, const unsigned char* id, CommOwner* out, std::string* err);
int comm_all_gather(Comm* c, const void* send, void* recv, size_t bytes, hipStream_t s, std::string* err);
void comm_info(const Comm* c, int* rank, int* world);
// Solves window k (desc row d) of the batch on stream s; writes b.x / b.y / b.stats / b.istats of window k.
hipError_t large_solve(LargeSolver* ls, const Batch& b, int k, const int64_t* d, const Opts& o, const double* hinv,
                       hipStream_t s, std::string* err, float* setup_ms, float* pdhg_ms);

// The band kernel's interconnection form (dvh_band_grid.hip; dvh_set_kernel_path 5): battery windows with POI limit
// rows, a curtailable-PV column block and / or charge-from-PV rows, one workgroup per listed window.  A workgroup
// returns at once unless its window's status is -2 (kNeedsEll), so the launch follows the ICE pass over the same
// list; windows it refuses keep status -2.  variant_out: 9000000 + 200 + waves per window.  early: as launch_pdhg's.
hipError_t launch_pdhg_band_grid(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                                 const int32_t* list, int nlist, int* variant_out, int32_t* early = nullptr);

// The band kernel's load-shift form (dvh_band_shift.hip; dvh_set_kernel_path 6): battery windows with a controllable
// load (two more column blocks pw, el and T + D more equality rows), one workgroup per listed window.  As the
// interconnection form, a workgroup returns at once unless its window's status is -2 (kNeedsEll), so the launch follows
// the ICE pass over the same list; windows it refuses keep status -2.  variant_out: 9000000 + 300 + waves per window.
hipError_t launch_pdhg_band_shift(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                                  const int32_t* list, int nlist, int* variant_out);

// The band kernel's heat form (dvh_band_heat.hip; dvh_set_kernel_path 7): battery windows with one combined-heat-and-power
// unit (four more column blocks elec, on, steam, hotwater; T heat rows after the battery's T + 1; per step two generator
// rows and one ratio row among the >= rows), one workgroup per listed window.  gate: as the load-shift form, a workgroup
// returns at once unless its window's status is -2 (kNeedsEll), so the launch follows the ICE pass over the same list;
// without it every listed window is examined (solve_packed's launch over the heat-sized windows above kSmallMax).
// Windows it refuses have status -2.  variant_out: 9000000 + 400 + waves per window.
hipError_t launch_pdhg_band_heat(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                                 const int32_t* list, int nlist, int* variant_out, bool gate = true);
// The descriptor's sizes are those of a window the heat form can hold (m_eq = 2 T + 1, T <= 768, n = 7 T + J, J <= 4,
// 3 T .. 4 T >= rows): its largest windows are above kSmallMax (n = 5,380, m = 4,609).
bool band_heat_sized(int64_t n, int64_t m, int64_t meq);

// Certificate pass (dvh_certify.hip; dvh_options.certify, dvh_certify_batch): plain PDHG on the unscaled LP of every
// on-chip window of the batch, one workgroup each, until a Farkas certificate (status 1, the ray in y) or an unbounded
// ray (status 2, the ray in x) passes its test or `cap` iterations are done.  gate != 0 (after a solve): a workgroup
// leaves at once unless its window's status is ITER_LIMIT or NUMERICAL, and a window that is not certified is left
// exactly as it was; gate == 0 (the screen): every window, the undecided ones come back with status 5 (DVH_UNDECIDED).
// The workspace is the pass's own, indexed by the descriptors' offsets less window 0's (base_*): K' (tptr one extra
// entry per window), the steps, the last-step candidates.  counts[5] (device, zeroed by the caller) = {windows
// examined, primal infeasible, dual infeasible, skipped for size (n or m > kSmallMax), largest certificate-iteration
// count}.  max_n, max_m: the largest on-chip window (the launch's LDS).
//
// dvh_options.certify = 2 adds the early exit inside the PDHG kernels that take POI windows (pdhg_kernel, every
// instantiation; pdhg_band_grid_kernel), a compile-time flag on both, so levels 0 and 1 launch the instantiations they
// always did.  At every KKT check, before the termination test, the scaled dual y~ of T(z_k) is put through the pass's
// Farkas test.  With v = Dr y~ and kty = K~'y~ (which the check forms anyway; K~ = Dr K Dc, q~ = Dr q, l~ = l / Dc,
// u~ = u / Dc) every term of the margin is scale-free:
//     q'v = sum_i q~_i y~_i,   r = K'v = kty / Dc,   u_j r_j = u~_j kty_j,   l_j r_j = l~_j kty_j,
// and only viol = max |kty_j| / Dc_j, over the columns whose bound on r_j's side is infinite (the tau columns of the
// battery forms), needs a factor.  The >= rows of y~ are >= 0 by the projection.  The three conditions (margin > 0,
// viol <= 1e-8 margin, margin >= 1e-9 (sum |q~_i y~_i| + sum |bound terms|)) are homogeneous in v, so v is normalised
// only when they pass.  The sums and the maximum are block-reduced in a fixed order (no floating-point atomics), the
// decision is uniform across the workgroup and every wave leaves at the same barrier.  A certified window gets what
// the pass writes: status PRIMAL_INFEASIBLE, iters = the iteration of that check, y = v / ||v||_inf, stats {+inf,
// margin, viol, 0} recomputed for that y with the double factors and the window's own q, l, u; x is the last checked
// candidate and means nothing.  One lane adds the window to the handle's early counters {windows, largest iteration
// count} (dvh_last_certify_early), which travel to the host with the pass's pinned word.  The pass still follows the
// solve and skips such a window by its status.  The band, ICE, ELL, chain and grid-wide tiers ignore the level: their
// windows keep the pass.  Unbounded rays are not tested in the kernels: dual-infeasible windows keep the pass too.
constexpr int kCertifyDefaultCap = 65536;
struct CertWork {
  int32_t* tptr;   // [sum n + count]
  int32_t* tind;   // [sum nnz]
  double* tval;    // [sum nnz]
  double* tau;     // [sum n]
  double* gx;      // [sum n]
  double* sig;     // [sum m]
  double* gy;      // [sum m]
  int32_t* counts; // [5]
  int64_t base_n, base_m, base_nz;
};
size_t certify_lds_bytes(int max_n, int max_m);
hipError_t launch_certify(const Batch& b, const CertWork& cw, int count, int max_n, int max_m, int cap, int gate,
                          hipStream_t s);

}  // namespace dvh
