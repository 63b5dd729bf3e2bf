// dvh_band.hip -- PDHG kernel for the battery-banded window LP (gfx950), the DER-VET hot path's common shape.
//
// Same algorithm, scaling and check logic as pdhg_ell_kernel (dvh_kernels.hip; restated in oracle/pdlp_ref.py),
// for windows whose CSR is the storagevet battery + DCM window (dervet/MicrogridScenario.py:319 solves it per
// window; SURVEY.md Appendix A, dervet_hip/lp/builder.py), optionally with an LP-relaxed ICE (ICE = true):
//   x = [ch(T), dis(T), ene(T), tau(J)] (+ [elec(T), on(T)]),  J <= 4 demand periods in the window
//   row 0          ene_0                                      (= target)
//   row t+1        ch_t, dis_t, ene_t, ene_{t+1}               t = 0 .. T-2  (SOE recurrence)
//   row T          ch_{T-1}, dis_{T-1}, ene_{T-1}              (end-of-window target)
//   >= rows        ch_t, dis_t, tau_j (+ elec_t)               at most one per step t (DCM epigraph)
//   >= rows (ICE)  elec_t, on_t                                exactly two per step (rated / minimum power,
//                                                              RotatingGeneratorSizing.py:110-136)
//   bounds         ch, dis (, elec, on) >= 0 (scaled lower bound exactly 0)
// The structure is detected and verified on the device from the CSR pattern (any values, any entry order
// within a row, >= rows in any order); a window that does not match comes back with status kNeedsEll.
//
// Mapping: B lanes per window, lane l owns the S consecutive time steps S l .. S l + S - 1 -- their columns, their
// SOE / DCM (/ ICE) rows -- with every coefficient, bound, objective, iterate and anchor in VGPRs.  An SpMV needs
// only the next step's ene (K x) and the previous SOE row's dual (K^T y); inside a lane those are registers, across
// lanes one LDS store + one LDS load per lane and half-step.  The dense tau columns are summed by wave 0 from
// per-lane partials.  Three forms are instantiated (launch_pdhg_band, at the end of the file):
//   <256, 3> battery  three steps per lane, 4 waves = one per SIMD, about 252 VGPRs (2 waves per SIMD), costs and
//                     right-hand sides in LDS: two windows share a CU, so one window's barrier waits are filled by the
//                     other's work.  The default; persistent grid (dvh_band_persist.hip), which also has the form's
//                     single-demand-period instantiation (band_window, J1) for lists whose windows all have J == 1.
//   <768, 1> battery  one step per lane, 12 waves, one window per CU: batches of at most one window per CU
//                     (dvh_api.cpp picks the form by batch size), one workgroup per window.
//   <768, 1> ICE      one step per lane at a 168-VGPR budget (3 waves per SIMD; twice the per-step state, the ICE
//                     columns' and rows' read-only data in LDS).  Persistent grid (dvh_band_persist_ice.hip).
// What was measured and not kept in this kernel is listed in DESIGN.md section 4, "Measured and not kept (band kernel)".
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "dvh_device.h"

namespace dvh {
namespace {

constexpr int kBandSteps = 768;  // steps per window (T <= kBandSteps)
constexpr int kJMax = kBandJMax;  // tau (demand-period) columns per window
constexpr int kNeedsEll = -2;

// LDS layout (B lanes, S steps per lane, SB = S B steps; NC / NR = columns / rows per step), doubles then ints:
//   XE[B+1] YS[B+1] XT[kJMax] red[kNRed(NW+1)+4] TP[kJMax][B] XP[NC S][B] YP[NR S][B] (ICE: RO[6 S][B]) (LC: CQ[5 S][B])
//   | ints: dcm[SB] ice_a[SB] ice_b[SB] ice_n[SB] flag[4] | DRL[S][B]
// LC (the three-step form): CQ = c of ch / dis / ene and q of the SOE / DCM rows in LDS instead of VGPRs (one FMA
// addend per iteration), and the ints, read only during the set-up, share the check images' space XP / YP, so that two
// windows fit one CU's LDS.  DRL: the lane's DCM row indices, kept in LDS from the set-up to the write-back (held in
// VGPRs across the iteration loop they were among the persistent form's spilled values).
__host__ __device__ constexpr size_t band_lds_doubles(int B, int S, bool ice, bool lc) {
  const int NW = B / kWave, NC = ice ? 5 : 3, NR = ice ? 4 : 2;
  const size_t SB = (size_t)S * B;
  return 2 * (size_t)(B + 1) + kJMax + (size_t)kNRed * (NW + 1) + 4 + (size_t)kJMax * B + (NC + NR) * SB +
         (lc ? 5 * SB : 0) + (ice ? 6 * SB : 0);
}
__host__ __device__ constexpr size_t band_ints_bytes(int B, int S) { return sizeof(int32_t) * (4 * (size_t)S * B + 4); }
__host__ __device__ constexpr size_t band_drow_bytes(int B, int S) { return align16(sizeof(int32_t) * (size_t)S * B); }
__host__ __device__ constexpr size_t band_lds_bytes(int B, int S, bool ice, bool lc) {
  const size_t d = align16(sizeof(double) * band_lds_doubles(B, S, ice, lc));
  return (lc ? d : d + align16(band_ints_bytes(B, S))) + band_drow_bytes(B, S);
}
static_assert(band_lds_bytes(kBandSteps / 3, 3, false, true) == 77328, "three-step battery form: two windows per CU");
static_assert(band_lds_bytes(kBandSteps, 1, false, false) == 84192, "one-step battery form");
static_assert(band_lds_bytes(kBandSteps, 1, true, false) == 145632, "ICE form");

// How the forms differ: the ICE form (168-VGPR budget, already spilling) from the battery forms, and the three-step
// battery form (S = 3, the bench's) from the one-step one.
template <bool ICE, int S>
struct BandTune {
  // the KKT helpers below inlined into the check (out of line every call binds the caller's live registers to the call
  // ABI; battery +0.8-1.5 %, profiles/r05s_check_cost_*.log; ICE -5.6 % inlined, profiles/r05za_config5_bisect.log)
  static constexpr bool kkt_inline = !ICE;
  // a check's single-precision factors loaded together at its top, one wait instead of 15 serialised global-memory
  // latencies (ICE: 14 more spilled VGPRs, config 5 111.9k vs 114.7k windows/s, profiles/r06c_ab.log)
  static constexpr bool kkt_prefetch = !ICE;
  // the waves without the tau column finish their own-column K x-bar before the first barrier, where they wait for
  // wave 0 anyway (ICE 116.5k -> 126.0k; battery within its spread at +10 spilled VGPRs, profiles/r06l_pin_kx.log)
  static constexpr bool pin_kx = ICE;
  // the check path's wave-uniform doubles through v_readfirstlane, held in SGPR pairs between checks (ICE spills
  // 41 -> 19, config 5 +1.3 %, profiles/r06r_uscal.log; the three-step battery form with the plain-iteration loop
  // spills 47 -> 22 VGPRs, bench 371.6 -> 363.9 ms per step, profiles/band_loop_variants.log -- before that loop it
  // ran 1.8 % slower with them; the one-step battery form keeps its VGPR copies)
  static constexpr bool uniform_check_scalars = ICE || S == 3;
  // the objective gate's dual-residual term sum_j |r_d,j| |x_j| (kkt_done; the extra reduced value cost the ICE form
  // 6 % on config 5 at unchanged iterations, profiles/r04ab_ab_kkt_rdx.log: its windows keep the round-3 test)
  static constexpr bool gate_rdx = !ICE;
  // the plain iterations between two checks in an innermost loop of their own, one per wave kind (see the solve loop):
  // three-step battery form bench 392.6-394.7 -> 371.5-371.7 ms per step, one-step battery form config 1 13.1k -> 15.7k
  // and config 2 15.0-15.2k -> 16.8-16.9k windows/s; the ICE form spills 66 VGPRs instead of 19 with it and ran
  // config 5 at 131.0k against 131.2k windows/s (profiles/band_loop_variants.log)
  static constexpr bool plain_loop = !ICE;
  // wave 0's dual half-step: its LDS reads -- the next lane's ene, the tau x-bar and, for the init row, ene_0 -- in
  // front of the s_setprio 0 behind the first barrier, and the init row's lane-masked block without a read and a wait
  // of its own (see the dual half-step).  Bench -3.5 % per step; the early ene_0 alone -2 %, the reads in front of
  // s_setprio alone within the spread (profiles/band_w0_bench_ab.log).  The other forms keep their machine code.
  static constexpr bool w0_reads_first = !ICE && S == 3;
  // wave 0's plain iteration: the SOE rows of the lane's steps 0 .. S - 2 behind the second barrier, as on the other
  // waves, and no blend pinned in front of that barrier.  Wave 0 is the last wave there and waits 375 cycles at the
  // first (profiles/band_reads_latency.log), so the 33 FP64 instructions leave the span where it is critical.  Alone:
  // bench 343.1-345.3 against the parent's 345.4-346.0 ms per step, inside the spread; it is kept for what it gives
  // together with reads_ahead (profiles/band_reads_bench_ab.log).  Check iterations keep the parent's order, in which
  // their movement sums are accumulated.
  static constexpr bool w0_late = !ICE && S == 3;
  // every wave's plain iteration: the LDS reads of the next primal half-step (YS[tid], the nine costs, wave 0's four tau
  // partials) issue directly behind the second barrier and are carried across the loop's back edge in registers; the
  // x blends and the late rows run under their latency, and the reads' first use follows that block (see the end of
  // iterate).  With w0_late: bench 337.9-338.5 against the parent's 344.7-345.7 ms per step, 17 spilled VGPRs as before
  // (profiles/band_reads_bench_ab.log, band_reads_shape.txt).
  static constexpr bool reads_ahead = !ICE && S == 3;
};
// (BandTune::reads_ahead) What a plain iteration's primal half-step reads from LDS -- YS[tid], the lane's nine costs, on
// wave 0 the four tau partials -- is read behind the second barrier of the iteration before it (in front of the loop for
// its first trip; the last trip's reads are not used: the check iteration reads for itself) and carried across the back
// edge in this object's registers.  YS and TP are written in front of the second barrier and next behind the first, the
// costs at the set-up only, so the values are the ones the iteration's own reads would return.  hold(), at the
// iteration's end, keeps the compiler from sinking the reads back to their users at the loop's head; the wait it implies
// has the blend block in front of it.  The live range is that block: 10 VGPR pairs, 14 on wave 0.
template <int B, int S>
struct BandAhead {
  static constexpr int NW = B / kWave;
  const double *tp, *ys, *cq;  // TP + lane, YS + tid, CQ + tid (LDS)
  double y, c[S][3], t[NW];
  double xb[S][3];  // x-bar of the battery columns, for the blends behind the second barrier
  template <bool W0>
  __device__ __forceinline__ void read() {
    if constexpr (W0) {
#pragma unroll
      for (int r = 0; r < NW; ++r) t[r] = tp[r * kWave];
    }
    y = *ys;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int v = 0; v < 3; ++v) c[s][v] = cq[(v * S + s) * B];
  }
  template <bool W0>
  __device__ __forceinline__ void hold() {
    if constexpr (W0) {
#pragma unroll
      for (int r = 0; r < NW; ++r) t[r] = opaque(t[r]);
    }
    y = opaque(y);
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int v = 0; v < 3; ++v) c[s][v] = opaque(c[s][v]);
  }
};
struct BandNoAhead {};
// Wave 0, whose primal half-step carries the tau column's reduction and update, runs that half-step at this s_setprio
// level, so that the SIMD it shares with the other window's wave issues its instructions first (profiles/r06a_ab.log).
// Wave 0 is no longer the wave the others wait for at the first barrier -- it waits there itself, for waves 1-3
// (profiles/band_reads_latency.log) -- but the raise still pays: on top of w0_late and reads_ahead, no raised priority
// ran the bench at 350.2-350.7 ms per step, level 1 at 337.9-338.1, the raise ended at the tau reduction's last DPP
// level at 346.7-348.2, against 337.3-339.2 for this (profiles/band_reads_bench_ab.log).
constexpr int kTauWavePrio = 2;

// KKT pieces of one column / one row.  Scale-free where the check compares large terms: the objectives' sums c'x, q'y
// and the bound term l'lam+ + u'lam- are the same in the scaled space (c~ x~ = c x, l~ lam~ = (l / d)(d lam) with
// lam~ = c~ - K~'y~ the scaled reduced cost, d > 0 keeping its sign), so the gap needs no factor at all.  Only the
// residual norms and ||y|| are unscaled, with fd = the factor in single precision (Work::fc / fr) and a 1-ulp
// v_rcp_f32 reciprocal: each term moves by a relative 2e-7 at most, i.e. each norm by a relative 2e-7 of itself.  The
// outputs are unscaled with the exact factors.
// _i: inlined (BandTune::kkt_inline); _o: out of line, so that the check does not raise the kernel's register allocation.
struct ColKkt {
  double rd2, cx, bt;
};
struct ColKktX : ColKkt {
  double rdx;  // |r_d| |x| of the column, unscaled (BandTune::gate_rdx)
};
__device__ __noinline__ ColKkt col_kkt_o(double kt, double cj, double loj, double hij, double xj, float fd) {
  const double id = (double)__builtin_amdgcn_rcpf(fd);
  const double rs = cj - kt;  // scaled reduced cost
  const bool fl = isfinite(loj), fh = isfinite(hij);
  const double lam = (fl && fh) ? rs : (fl ? fmax(rs, 0.0) : (fh ? fmin(rs, 0.0) : 0.0));
  const double rd = (rs - lam) * id;
  return {rd * rd, cj * xj, (fl ? loj * fmax(lam, 0.0) : 0.0) + (fh ? hij * fmin(lam, 0.0) : 0.0)};
}
__device__ __forceinline__ ColKktX col_kkt_x_i(double kt, double cj, double loj, double hij, double xj, float fd) {
  const double id = (double)__builtin_amdgcn_rcpf(fd);
  const double rs = cj - kt;  // scaled reduced cost
  const bool fl = isfinite(loj), fh = isfinite(hij);
  const double lam = (fl && fh) ? rs : (fl ? fmax(rs, 0.0) : (fh ? fmin(rs, 0.0) : 0.0));
  const double rd = (rs - lam) * id;
  ColKktX r;
  r.rd2 = rd * rd;
  r.cx = cj * xj;
  r.bt = (fl ? loj * fmax(lam, 0.0) : 0.0) + (fh ? hij * fmin(lam, 0.0) : 0.0);
  r.rdx = fabs(rd) * fabs(xj * (double)fd);
  return r;
}
struct RowKkt {
  double rp2, y2;
};
__device__ __forceinline__ RowKkt row_kkt_i(double kv, double qi, double yi, float fd, int ge) {
  const double dr = (double)fd, idr = (double)__builtin_amdgcn_rcpf(fd);
  double r = (qi - kv) * idr;
  if (ge) r = fmax(r, 0.0);
  return {r * r, (yi * dr) * (yi * dr)};
}
__device__ __noinline__ RowKkt row_kkt_o(double kv, double qi, double yi, float fd, int ge) {
  return row_kkt_i(kv, qi, yi, fd, ge);
}
template <bool INL>
__device__ __forceinline__ RowKkt row_kkt_fn(double kv, double qi, double yi, float fd, int ge) {
  if constexpr (INL) return row_kkt_i(kv, qi, yi, fd, ge);
  else return row_kkt_o(kv, qi, yi, fd, ge);
}

// GATE: the predicted KKT gate (dvh_options.kkt_predict > 0) is compiled in only where the host asks for it -- its
// state and extra reduction raised the register allocation of the check path by 30-40 spilled VGPRs in every form
// (profiles/r02zzk_ab_configs12_spills.log), which runs with the default options paid for nothing.
//
// BOX (box form, the default): every ch / dis / ene (/ elec / on) column has a finite box [lo, hi] in the
// scaled space, so the kernel iterates on x' = (x - lo) / w, w = hi - lo, whose box is [0, 1]: the projection is the
// FMA's own clamp modifier (one v_fma_f64 ... clamp instead of v_fma + v_max + v_min per column and iteration).  The
// change of variables is exact: K' = K diag(w) (both SpMV directions), c' = c w, q' = q - K lo, and a per-column
// primal step tau / w^2 gives x' + (tau / w^2)(w g) = (x + tau g - lo) / w, i.e. the same PDHG iterates.  The
// movement norms that drive restarts and the primal weight are taken in x units (w d'), the KKT check runs on the
// primed LP, whose objectives, row residuals and (zero, for a two-sided box) column residuals equal the original's
// once the constant c lo is added.  A window with an unbounded ch / dis / ene (/ elec / on) column is returned with
// status kNeedsPlain and re-run by the plain form (dvh_api.cpp device_cascade).
// The widths w are kept nowhere: the per-column steps tau / w^2 are formed from the registers at the box set-up, a
// restart rescales them by tau_new / tau_old (one uniform quotient, no per-column division), the check iteration's
// movement norms weigh each column's d'^2 by w^2 = tau / step (an approximate reciprocal: the norms only steer restarts
// and the primal weight), and the write-back recomputes w = u / d - l / d with the set-up's operations (bit-identical).
constexpr int kNeedsPlain = -3;
// DVH_BAND_PROBE (A/B builds only, scripts/probe_band_latency.py): every wave accumulates the shader-clock cycles of
// its iterations' seven segments -- primal half-step, wait at the first barrier, dual half-step up to the init row, the
// init row's block (lane kInitLane of wave 0; next to nothing on the other waves), what is left in front of the second
// barrier (the blends, where they are placed there), the wait at the second barrier, what follows it up to the
// iteration's end (late rows, blends placed there) -- and of the checks, and lane 0 writes them over
// x[9 wid .. 9 wid + 7] of its window at the end, with the wave's HW_ID register (SIMD, CU, SE, workgroup slot) in
// x[9 wid + 8].
#ifndef DVH_BAND_PROBE
#define DVH_BAND_PROBE 0
#endif
__device__ __forceinline__ unsigned long long probe_clock() {
#if DVH_BAND_PROBE
  return __builtin_amdgcn_s_memtime();
#else
  return 0ull;
#endif
}
__device__ __forceinline__ double fma_clamp01(double a, double b, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// a check-path wave-uniform double, made scalar where BandTune says so (USC = BandTune::uniform_check_scalars)
template <bool USC>
__device__ __forceinline__ double usc(double v) {
  return USC ? uniform(v) : v;
}
// a uniform double the optimiser must re-read where it is used (so that what is formed from it is not hoisted out of the
// iteration loop into a long-lived VGPR pair)
template <bool USC>
__device__ __forceinline__ double sgpr_fresh(double v) {
  if constexpr (USC) asm volatile("" : "+s"(v));
  return v;
}
// J1: the single-demand-period instantiation (three-step battery form): J is the constant 1 through the whole window, so
// the set-up's, the checks' and the write-back's loops over the tau columns are straight-line code, and the waves
// without the tau column (wave 0 is the tau wave of every window) carry no tau update, no init row, no period index per
// step and read XT[0] once per dual half-step.  The arithmetic and its order are those of the run-time J == 1 path.  The
// host launches it only for lists without a J != 1 battery window (launch_pdhg_band, j1); a window whose descriptor
// says otherwise leaves through bail() with the first test, before any shared state is written.
template <int B, int S, bool ICE, bool LC, int WPS, bool GATE, bool BOX, bool J1 = false>
__device__ __forceinline__ void band_window(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, const int k_in,
                                            const int tid) {
  // the window index and its descriptor's offsets through v_readfirstlane, so that they and every address formed from
  // them (the window's CSR, costs, bounds, outputs, workspace) are scalar: loaded as they are -- with vector loads, since
  // the kernel writes global memory the compiler does not treat the descriptors as constant -- they sat in VGPR pairs,
  // and the base addresses the set-up and the write-back use were spilled
  const int k = __builtin_amdgcn_readfirstlane(k_in);
  using Tune = BandTune<ICE, S>;
  constexpr bool USC = Tune::uniform_check_scalars;
  constexpr int NW = B / kWave;
  constexpr int SB = S * B;        // step capacity
  constexpr int NC = ICE ? 5 : 3;  // columns per step: ch, dis, ene (, elec, on)
  constexpr int NR = ICE ? 4 : 2;  // rows per step: SOE, DCM (, ICE rated, ICE minimum)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int kl = k - ch.first;
  const WinOff W = uniform_win(win_offsets(b, ch, k));
  const int n = W.n, m = W.m, meq = W.meq;
  const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* scal = w.scal + (int64_t)kl * kScal;
  static_assert(!(J1 && ICE), "the single-demand-period instantiation is a battery form");
  const int T = meq - 1, JD = n - (ICE ? 5 : 3) * T, J = J1 ? 1 : JD, MI = m - meq;
  const int MD = ICE ? MI - 2 * T : MI;  // DCM rows
  auto bail = [&]() {
    if (tid == 0) {
      b.istats[2 * k] = kNeedsEll;
      b.istats[2 * k + 1] = 0;
    }
  };
  // the kernel scales its windows itself (below): it runs before, and instead of, setup_kernel, whose outputs it
  // does not read; the windows it hands on are set up after it (dvh_api.cpp device_cascade)
  if (n > kSmallMax || m > kSmallMax || T < 1 || T > SB || JD < 0 || JD > kJMax || MD < 0 || MD > T ||
      (JD == 0 && MD > 0) || (J1 && JD != 1)) {
    bail();
    return;
  }
  const int CE = 3 * T + J, CO = 4 * T + J;  // first elec / on column (ICE)
  // ---- LDS carve
  double* XE = reinterpret_cast<double*>(smem);  // x-bar (x+) of ene of lane l's first step at [l]; [B] stays 0
  double* YS = XE + (B + 1);  // y (y+) of the init row at [0], of the SOE row of lane l's last step at [l + 1]
  double* XT = YS + (B + 1);  // x-bar (x+) of the tau columns
  double* red = XT + kJMax;
  double* TP = red + kNRed * (NW + 1) + 4;  // [kJMax][B] per-lane partial K'y of the tau columns
  double* XP = TP + kJMax * B;  // [NC S][B] T(z) of the lane's columns (check iterations)
  double* YP = XP + NC * SB;    // [NR S][B] T(z) of the lane's rows
  // ICE: read-only data of the ICE columns / rows in LDS instead of VGPRs (the register budget at 3 waves per
  // SIMD is 168): RO[0..1] = c of elec / on, RO[2..3] = upper bound of elec / on, RO[4..5] = q of the two ICE rows,
  // each [S][B]
  double* RO = YP + NR * SB;
  double* CQ = RO + (ICE ? 6 * SB : 0);  // [5 S][B] (LC)
  static_assert(sizeof(double) * (NC + NR) * SB >= band_ints_bytes(B, S), "the ints fit the images");
  int32_t* dcm = LC ? reinterpret_cast<int32_t*>(XP)  // (LC) the ints share the images' LDS
                    : reinterpret_cast<int32_t*>(smem + align16(sizeof(double) * band_lds_doubles(B, S, ICE, LC)));
  int32_t* ice_a = dcm + SB;  // [SB] ICE rows of each step (lower / higher row index), and their count
  int32_t* ice_b = ice_a + SB;
  int32_t* ice_n = ice_b + SB;
  int32_t* flag = ice_n + SB;
  int32_t* DRL = reinterpret_cast<int32_t*>(smem + band_lds_bytes(B, S, ICE, LC) - band_drow_bytes(B, S));  // [S][B]

  const int32_t* gkp = b.indptr + W.row;
  const int32_t* gkc = b.indices + W.nz;
  const double* gkv = b.data + W.nz;  // the window's own (unscaled) data
  const double* craw = b.c + W.on;
  const double* lraw = b.l + W.on;
  const double* uraw = b.u + W.on;
  const double* qraw = b.q + W.om;
  double* dcv = w.dc + W.wn;  // the factors this kernel computes (the outputs are unscaled with them)
  double* drv = w.dr + W.wm;
  // the factor of column j / row i at the write-back (kept as lambdas: with plain dcv[j] / drv[i] there the one-step
  // battery kernels come out with two SGPRs exchanged, and the certified machine code is kept bit for bit)
  auto dcf = [&](int j) -> double { return dcv[j]; };
  auto drf = [&](int i) -> double { return drv[i]; };
  double* xo_g = b.x + W.on;
  double* yo_g = b.y + W.om;

  // ---- structure check (every entry of every row accounted for) and the step -> row maps
  for (int u = tid; u < SB; u += B) {
    dcm[u] = -1;
    ice_a[u] = 0x7fffffff;
    ice_b[u] = -1;
    ice_n[u] = 0;
  }
  if (tid == 0) flag[0] = flag[1] = flag[2] = 0;
  __syncthreads();
  int bad = 0, crossed = 0, unboxed = 0;
  for (int j = tid; j < J; j += B) crossed |= lraw[3 * T + j] > uraw[3 * T + j];
  for (int r = tid; r <= T; r += B) {
    const int p0 = gkp[r], len = gkp[r + 1] - p0;
    if (r == 0) {
      bad |= !(len == 1 && gkc[p0] == 2 * T);
      continue;
    }
    const int t = r - 1;
    if (len != (r < T ? 4 : 3)) {
      bad = 1;
      continue;
    }
    unsigned seen = 0;
    for (int e = 0; e < len; ++e) {
      const int c = gkc[p0 + e];
      const int kind = c == t ? 0 : c == T + t ? 1 : c == 2 * T + t ? 2 : (r < T && c == 2 * T + t + 1) ? 3 : 4;
      if (kind == 4 || ((seen >> kind) & 1u)) bad = 1;
      seen |= 1u << kind;
    }
    // the kernel keeps no lower bound for ch / dis (/ elec / on); crossed bounds: infeasible as given
    bad |= lraw[t] != 0.0 || lraw[T + t] != 0.0;
    crossed |= lraw[t] > uraw[t] || lraw[T + t] > uraw[T + t] || lraw[2 * T + t] > uraw[2 * T + t];
    if (BOX) unboxed |= !(isfinite(uraw[t]) && isfinite(uraw[T + t]) && isfinite(lraw[2 * T + t]) && isfinite(uraw[2 * T + t]));
    if (ICE) {
      if (BOX) unboxed |= !(isfinite(uraw[CE + t]) && isfinite(uraw[CO + t]));
      bad |= lraw[CE + t] != 0.0 || lraw[CO + t] != 0.0;
      crossed |= lraw[CE + t] > uraw[CE + t] || lraw[CO + t] > uraw[CO + t];
    }
  }
  for (int i = meq + tid; i < m; i += B) {
    const int p0 = gkp[i], len = gkp[i + 1] - p0;
    if (ICE && len == 2) {  // ICE row: elec_t, on_t
      int te = -1, to = -1;
      for (int e = 0; e < 2; ++e) {
        const int c = gkc[p0 + e];
        if (c >= CE && c < CE + T) te = c - CE;
        else if (c >= CO && c < CO + T) to = c - CO;
      }
      if (te < 0 || te != to) {
        bad = 1;
        continue;
      }
      atomicMin(&ice_a[te], i);
      atomicMax(&ice_b[te], i);
      atomicAdd(&ice_n[te], 1);
      continue;
    }
    if (len != (ICE ? 4 : 3)) {
      bad = 1;
      continue;
    }
    int tc = -1, td = -1, jj = -1, te = ICE ? -1 : -2;
    for (int e = 0; e < len; ++e) {
      const int c = gkc[p0 + e];
      if (c < T) {
        bad |= tc >= 0;
        tc = c;
      } else if (c < 2 * T) {
        bad |= td >= 0;
        td = c - T;
      } else if (c >= 3 * T && c < 3 * T + J) {
        bad |= jj >= 0;
        jj = c - 3 * T;
      } else if (ICE && c >= CE && c < CE + T) {
        bad |= te >= 0;
        te = c - CE;
      } else {
        bad = 1;
      }
    }
    if (tc < 0 || td != tc || jj < 0 || (ICE && te != tc)) {
      bad = 1;
      continue;
    }
    if (atomicCAS(&dcm[tc], -1, i * 8 + jj) != -1) bad = 1;  // at most one DCM row per step
  }
  if (bad) flag[0] = 1;
  if (crossed) flag[1] = 1;
  if (unboxed) flag[2] = 1;
  __syncthreads();
  if (ICE)
    for (int u = tid; u < T; u += B)
      if (ice_n[u] != 2) flag[0] = 1;  // exactly two ICE rows per step
  __syncthreads();
  if (flag[1] != 0) {  // crossed bounds, reported as setup_kernel reports them (no iterations)
    if (tid == 0) {
      scal[0] = 0.0;
      scal[6] = 3.0;
      b.istats[2 * k] = 1;  // DVH_PRIMAL_INFEASIBLE
      b.istats[2 * k + 1] = 0;
      for (int u = 0; u < 4; ++u) b.stats[4 * k + u] = u == 0 ? NAN : 0.0;
    }
    return;
  }
  if (flag[0] != 0) {
    bail();
    return;
  }
  auto bail_plain = [&]() {
    if (tid == 0) {
      b.istats[2 * k] = kNeedsPlain;
      b.istats[2 * k + 1] = 0;
    }
  };
  if (BOX && flag[2] != 0) {
    bail_plain();
    return;
  }

  // ---- the lane's steps t = S tid + s: columns (v) ch, dis, ene (, elec, on), rows (r) SOE, DCM (, ICE a, ICE b)
  const int t0 = S * tid;
  bool val[S];
  double x[S][NC], xa[S][NC], cc[S][3], hi[S][3];
  double loe[S];                     // lower bound of ene (the others are 0)
  double ks[S][4];                   // SOE row: coefficients of ch_t, dis_t, ene_t, ene_{t+1}
  double kd[S][4];                   // DCM row: coefficients of ch_t, dis_t, tau_j, elec_t
  double ka[S][2], kb[S][2];         // ICE rows: coefficients of elec_t, on_t
  double kp0 = 0.0;                  // coefficient of ene_{t0} in row t0 (the init row or the previous lane's SOE
                                     // row); for s > 0 the coefficient of ene_t in row t is ks[s - 1][3]
  double y[S][NR], ya[S][NR], q[S][2];
  int drow[S], jt[S], ra[S], rb[S];
  auto col = [&](int s, int v) { return v < 3 ? v * T + t0 + s : (v == 3 ? CE : CO) + t0 + s; };
  auto ro = [&](int u, int s) -> double& { return RO[(u * S + s) * B + tid]; };
  auto cqa = [&](int u, int s) -> double& { return CQ[(u * S + s) * B + tid]; };
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int t = t0 + s;
    val[s] = t < T;
#pragma unroll
    for (int v = 0; v < NC; ++v) x[s][v] = xa[s][v] = 0.0;
#pragma unroll
    for (int v = 0; v < 3; ++v) cc[s][v] = hi[s][v] = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) y[s][r] = ya[s][r] = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) ks[s][u] = kd[s][u] = 0.0;
    ka[s][0] = ka[s][1] = kb[s][0] = kb[s][1] = 0.0;
    q[s][0] = q[s][1] = 0.0;
    loe[s] = 0.0;
    drow[s] = -1;
    DRL[s * B + tid] = -1;
    jt[s] = 0;
    ra[s] = rb[s] = -1;
    if (ICE)
      for (int u = 0; u < 6; ++u) ro(u, s) = 0.0;
    if (LC)
      for (int u = 0; u < 5; ++u) cqa(u, s) = 0.0;
  }
  auto cof = [&](int s, int v) -> double { return v < 3 ? (LC ? cqa(v, s) : cc[s][v]) : ro(v - 3, s); };
  auto qv = [&](int s, int r) -> double { return LC ? cqa(3 + r, s) : q[s][r]; };
  auto hib = [&](int s, int v) -> double { return v < 3 ? hi[s][v] : ro(v - 1, s); };
  auto rhs = [&](int s, int r) -> double { return r < 2 ? qv(s, r) : ro(r + 2, s); };
  // ---- the lane's coefficients (unscaled) and row maps
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (!val[s]) continue;
    const int t = t0 + s;
    for (int p = gkp[t + 1]; p < gkp[t + 2]; ++p) {
      const int c = gkc[p];
      const double a = gkv[p];
      if (c == t) ks[s][0] = a;
      else if (c == T + t) ks[s][1] = a;
      else if (c == 2 * T + t) ks[s][2] = a;
      else ks[s][3] = a;
    }
    if (s == 0)
      for (int p = gkp[t]; p < gkp[t + 1]; ++p)
        if (gkc[p] == 2 * T + t) kp0 = gkv[p];
    const int dv = dcm[t];
    if (dv >= 0) {
      drow[s] = dv >> 3;
      DRL[s * B + tid] = drow[s];
      jt[s] = J1 ? 0 : dv & 7;
      for (int p = gkp[drow[s]]; p < gkp[drow[s] + 1]; ++p) {
        const int c = gkc[p];
        const double a = gkv[p];
        if (c < T) kd[s][0] = a;
        else if (c < 2 * T) kd[s][1] = a;
        else if (c < 3 * T + J) kd[s][2] = a;
        else kd[s][3] = a;
      }
    }
    if (ICE) {
      ra[s] = ice_a[t];
      rb[s] = ice_b[t];
      for (int p = gkp[ra[s]]; p < gkp[ra[s] + 1]; ++p) (gkc[p] < CO ? ka[s][0] : ka[s][1]) = gkv[p];
      for (int p = gkp[rb[s]]; p < gkp[rb[s] + 1]; ++p) (gkc[p] < CO ? kb[s][0] : kb[s][1]) = gkv[p];
    }
  }
  // row of step s's r-th row (SOE, DCM, ICE a, ICE b), or -1 where the step has none
  auto row_of = [&](int s, int r) -> int {
    return r == 0 ? (val[s] ? t0 + s + 1 : -1) : r == 1 ? drow[s] : (val[s] ? (r == 2 ? ra[s] : rb[s]) : -1);
  };
  // Special state in wave 0 (registers sp[], meaning by lane): lane j < J holds tau column j {x, xa, c, lo, hi, x+};
  // lane kInitLane holds the init row (row 0: ene_0 = target) {y, ya, y+, q, coefficient, -}.
  constexpr int kInitLane = kWave - 1;
  static_assert(kJMax < kInitLane, "tau lanes and the init-row lane are distinct");
  const bool tlane = wid == 0 && lane < J, ilane = wid == 0 && lane == kInitLane;
  double sp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  // ---- scaling: setup_kernel's preconditioning (o.ruiz_iters Ruiz inf-norm passes, then one Pock-Chambolle
  //      alpha = 1 pass, row and column factors of a pass both from the same scaled matrix) restated on the band
  //      structure, every factor in the registers of the lane that owns the row / column: a row's entries are its
  //      step's columns (+ the next step's ene: the next lane's, through XE; + its period's tau: XT), a column's
  //      entries its step's rows (+ ene's previous SOE row: the previous lane's, through YS); the tau columns are
  //      reduced through TP by wave 0, whose lane j holds tau j's factor (fsp), as lane kInitLane holds the init row's.
  //      Factors 1 / sqrt(norm) by v_rsq_f64: a preconditioner needs no correctly rounded factor, and every scaled
  //      quantity is formed from the same stored factor that unscales the results.
  double fcv[S][NC], frv[S][NR], fsp = 1.0, kin0 = 0.0;  // kin0: the init row's coefficient (of ene_0)
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int v = 0; v < NC; ++v) fcv[s][v] = 1.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) frv[s][r] = 1.0;
  }
  if (ilane) kin0 = gkv[gkp[0]];
  auto factor = [](double a) { return a > 0.0 ? __builtin_amdgcn_rsq(a) : 1.0; };
  auto exchange = [&]() {
    XE[tid] = fcv[0][2];
    YS[tid + 1] = frv[S - 1][0];
    if (tid == 0) XE[B] = 1.0;  // (no step after the last lane's: its coefficient is 0)
    if (tid < kJMax) XT[tid] = tlane ? fsp : 1.0;
    if (ilane) YS[0] = fsp;
  };
  for (int pass = 0; pass <= o.ruiz_iters; ++pass) {
    const bool pc = pass == o.ruiz_iters;
    auto acc = [pc](double a, double v) { return pc ? a + v : fmax(a, v); };
    exchange();
    __syncthreads();
    const double fen = XE[tid + 1], frp = YS[tid];
    double nr[S][NR], nc[S][NC];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double fe1 = s < S - 1 ? fcv[s < S - 1 ? s + 1 : s][2] : fen;
      const double rp = s == 0 ? frp : frv[s > 0 ? s - 1 : 0][0];
      const double kpr = s == 0 ? kp0 : ks[s > 0 ? s - 1 : 0][3];
      const double r0 = frv[s][0], r1 = frv[s][1], ftj = XT[jt[s]];
      nr[s][0] = acc(acc(acc(fabs(ks[s][0]) * r0 * fcv[s][0], fabs(ks[s][1]) * r0 * fcv[s][1]),
                         fabs(ks[s][2]) * r0 * fcv[s][2]),
                     fabs(ks[s][3]) * r0 * fe1);
      nr[s][1] = acc(acc(fabs(kd[s][0]) * r1 * fcv[s][0], fabs(kd[s][1]) * r1 * fcv[s][1]), fabs(kd[s][2]) * r1 * ftj);
      nc[s][0] = acc(fabs(ks[s][0]) * r0 * fcv[s][0], fabs(kd[s][0]) * r1 * fcv[s][0]);
      nc[s][1] = acc(fabs(ks[s][1]) * r0 * fcv[s][1], fabs(kd[s][1]) * r1 * fcv[s][1]);
      nc[s][2] = acc(fabs(kpr) * rp * fcv[s][2], fabs(ks[s][2]) * r0 * fcv[s][2]);
      if constexpr (ICE) {
        const double r2 = frv[s][NR > 2 ? 2 : 0], r3 = frv[s][NR > 3 ? 3 : 0];
        const double f3 = fcv[s][NC > 3 ? 3 : 0], f4 = fcv[s][NC > 4 ? 4 : 0];
        nr[s][1] = acc(nr[s][1], fabs(kd[s][3]) * r1 * f3);
        nr[s][NR > 2 ? 2 : 0] = acc(fabs(ka[s][0]) * r2 * f3, fabs(ka[s][1]) * r2 * f4);
        nr[s][NR > 3 ? 3 : 0] = acc(fabs(kb[s][0]) * r3 * f3, fabs(kb[s][1]) * r3 * f4);
        nc[s][NC > 3 ? 3 : 0] = acc(acc(fabs(kd[s][3]) * r1 * f3, fabs(ka[s][0]) * r2 * f3), fabs(kb[s][0]) * r3 * f3);
        nc[s][NC > 4 ? 4 : 0] = acc(fabs(ka[s][1]) * r2 * f4, fabs(kb[s][1]) * r3 * f4);
      }
    }
    // tau columns: per-lane partials over the lane's DCM rows of each period (steps in order) -> wave 0
    for (int j = 0; j < J; ++j) {
      const double ftj = XT[j];
      double a = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (jt[s] == j) a = acc(a, fabs(kd[s][2]) * frv[s][1] * ftj);
      TP[j * B + tid] = a;
    }
    double nsp = 0.0;
    if (ilane) nsp = fabs(kin0) * fsp * XE[0];
    __syncthreads();
    if (wid == 0) {
      for (int j = 0; j < J; ++j) {
        double a = TP[j * B + lane];
#pragma unroll
        for (int r = 1; r < NW; ++r) a = acc(a, TP[j * B + r * kWave + lane]);
        a = uniform(pc ? wave_sum_dpp(a) : wave_max(a));
        if (lane == j) nsp = a;
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int v = 0; v < NC; ++v) fcv[s][v] *= factor(nc[s][v]);
#pragma unroll
      for (int r = 0; r < NR; ++r) frv[s][r] *= factor(nr[s][r]);
    }
    if (tlane || ilane) fsp *= factor(nsp);
    __syncthreads();  // every read of this pass's XE / YS / XT / TP is done
  }
  {  // the KKT checks unscale with single-precision copies of the factors: a window whose factors leave
     // [2^-100, 2^100] (far inside float's normal range) goes to the ELL / generic path, which keeps them in double
    auto oor = [](double f) { return !(f >= 0x1p-100 && f <= 0x1p100); };
    bool out = oor(fsp);
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int v = 0; v < NC; ++v) out |= oor(fcv[s][v]);
#pragma unroll
      for (int r = 0; r < NR; ++r) out |= oor(frv[s][r]);
    }
    if (__syncthreads_or(out)) {
      bail();
      return;
    }
  }
  exchange();
  __syncthreads();
  {  // scaled coefficients (K Dr) Dc, as setup_kernel forms them
    const double fen = XE[tid + 1], frp = YS[tid];
    kp0 = kp0 * frp * fcv[0][2];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double fe1 = s < S - 1 ? fcv[s < S - 1 ? s + 1 : s][2] : fen;
      const double r0 = frv[s][0], r1 = frv[s][1];
      ks[s][0] = ks[s][0] * r0 * fcv[s][0];
      ks[s][1] = ks[s][1] * r0 * fcv[s][1];
      ks[s][2] = ks[s][2] * r0 * fcv[s][2];
      ks[s][3] = ks[s][3] * r0 * fe1;
      kd[s][0] = kd[s][0] * r1 * fcv[s][0];
      kd[s][1] = kd[s][1] * r1 * fcv[s][1];
      kd[s][2] = kd[s][2] * r1 * XT[jt[s]];
      if constexpr (ICE) {
        const double r2 = frv[s][NR > 2 ? 2 : 0], r3 = frv[s][NR > 3 ? 3 : 0];
        const double f3 = fcv[s][NC > 3 ? 3 : 0], f4 = fcv[s][NC > 4 ? 4 : 0];
        kd[s][3] = kd[s][3] * r1 * f3;
        ka[s][0] = ka[s][0] * r2 * f3;
        ka[s][1] = ka[s][1] * r2 * f4;
        kb[s][0] = kb[s][0] * r3 * f3;
        kb[s][1] = kb[s][1] * r3 * f4;
      }
    }
    if (ilane) kin0 = kin0 * fsp * XE[0];
  }
  // ---- costs, bounds and right-hand sides, scaled (c Dc, l / Dc, u / Dc, q Dr); the factors for the outputs and
  //      the KKT checks; the norms for the primal weight and the relative KKT error
  double nrm[4] = {0.0, 0.0, 0.0, 0.0};  // ||c~||^2, ||q~||^2, ||c||^2, ||q||^2
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (!val[s]) continue;
    const int t = t0 + s;
#pragma unroll
    for (int v = 0; v < NC; ++v) {
      const int j = col(s, v);
      const double d = fcv[s][v], cj = craw[j];
      const double csj = cj * d, lsj = lraw[j] / d, usj = uraw[j] / d;
      if (v < 3) {
        hi[s][v] = usj;
        if (LC)
          cqa(v, s) = csj;
        else
          cc[s][v] = csj;
      } else {
        ro(v - 1, s) = usj;
        ro(v - 3, s) = csj;
      }
      if (v == 2) loe[s] = lsj;
      x[s][v] = xa[s][v] = fmin(fmax(o.warm ? xo_g[j] / d : 0.0, lsj), usj);
      nrm[0] += csj * csj;
      nrm[2] += cj * cj;
      dcv[j] = d;
      w.fc[W.wn + j] = (float)d;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = row_of(s, r);
      if (i < 0) continue;
      const double d = frv[s][r], qi = qraw[i], qsi = qi * d;
      if (r == 0) {
        if (LC)
          cqa(3, s) = qsi;
        else
          q[s][0] = qsi;
      } else if (r == 1) {
        if (LC)
          cqa(4, s) = qsi;
        else
          q[s][1] = qsi;
      } else {
        ro(r + 2, s) = qsi;
      }
      if (o.warm) y[s][r] = ya[s][r] = r == 0 ? yo_g[i] / d : fmax(yo_g[i] / d, 0.0);
      nrm[1] += qsi * qsi;
      nrm[3] += qi * qi;
      drv[i] = d;
      w.fr[W.wm + i] = (float)d;
    }
  }
  if (tlane) {
    const int j = 3 * T + lane;
    const double cj = craw[j], l0 = lraw[j] / fsp, h0 = uraw[j] / fsp;
    sp[0] = sp[1] = sp[5] = fmin(fmax(o.warm ? xo_g[j] / fsp : 0.0, l0), h0);
    sp[2] = cj * fsp;
    sp[3] = l0;
    sp[4] = h0;
    nrm[0] += sp[2] * sp[2];
    nrm[2] += cj * cj;
    dcv[j] = fsp;
    w.fc[W.wn + j] = (float)fsp;
  }
  if (ilane) {
    const double q0 = qraw[0];
    sp[3] = q0 * fsp;
    sp[4] = kin0;
    if (o.warm) sp[0] = sp[1] = sp[2] = yo_g[0] / fsp;
    nrm[1] += sp[3] * sp[3];
    nrm[3] += q0 * q0;
    drv[0] = fsp;
    w.fr[W.wm] = (float)fsp;
  }
  block_sum<B, 4>(nrm, red);
  const double ncs = sqrt(nrm[0]), nqs = sqrt(nrm[1]);
  const double pw0 = (ncs > 1e-10 && nqs > 1e-10) ? ncs / nqs : 1.0;  // setup_kernel's primal weight
  int xta[S];
#pragma unroll
  for (int s = 0; s < S; ++s) xta[s] = lds_addr(XT + jt[s]);
  if constexpr (LC) __syncthreads();  // the images overwrite the step -> row maps: every lane has read them
  // the check iterations' T(z) of the lane's columns / rows
  auto xpi = [&](int v, int s) -> double& { return XP[(v * S + s) * B + tid]; };
  auto ypi = [&](int r, int s) -> double& { return YP[(r * S + s) * B + tid]; };
  if (tid < kJMax) XT[tid] = 0.0;
  if (tid == 0) XE[B] = YS[B] = 0.0;
  XE[tid] = YS[tid] = 0.0;
  for (int u = tid; u < kJMax * B; u += B) TP[u] = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int v = 0; v < NC; ++v) xpi(v, s) = x[s][v];
#pragma unroll
    for (int r = 0; r < NR; ++r) ypi(r, s) = y[s][r];
  }
  __syncthreads();

  // ---- SpMV pieces (fixed summation order)
  auto kpv = [&](int s) { return s == 0 ? kp0 : ks[s > 0 ? s - 1 : 0][3]; };
  // K^T of step s's columns from its rows' values vr and vprev = the value of row t (the previous SOE row)
  auto ktr = [&](int s, const double (&vr)[NR], double vprev, double (&out)[NC]) {
    out[0] = fma(kd[s][0], vr[1], ks[s][0] * vr[0]);
    out[1] = fma(kd[s][1], vr[1], ks[s][1] * vr[0]);
    out[2] = fma(ks[s][2], vr[0], kpv(s) * vprev);
    if constexpr (ICE) {
      out[3] = fma(kb[s][0], vr[3], fma(ka[s][0], vr[2], kd[s][3] * vr[1]));
      out[4] = fma(kb[s][1], vr[3], ka[s][1] * vr[2]);
    }
  };
  // K of step s's rows, own-column part (kfin_next adds the next step's ene, kfin_tau the tau term)
  auto kown = [&](int s, const double (&v)[NC], double (&os)[NR]) {
    os[0] = fma(ks[s][2], v[2], fma(ks[s][1], v[1], ks[s][0] * v[0]));
    os[1] = fma(kd[s][1], v[1], kd[s][0] * v[0]);
    if constexpr (ICE) {
      os[1] = fma(kd[s][3], v[3], os[1]);
      os[2] = fma(ka[s][1], v[4], ka[s][0] * v[3]);
      os[3] = fma(kb[s][1], v[4], kb[s][0] * v[3]);
    }
  };
  auto kfin_next = [&](int s, double (&os)[NR], double vnext) { os[0] = fma(ks[s][3], vnext, os[0]); };
  auto kfin_tau = [&](int s, double (&os)[NR]) { os[1] = fma(kd[s][2], lds_ld(xta[s]), os[1]); };
  // The iteration's forms with the objective / right-hand side folded into the FMA chains: K^T y - c for the
  // primal half-step (x + tau (K^T y - c) = x - tau (c - K^T y)) and K x - q for the dual one (y - sigma (K x - q)):
  // one FP64 operation fewer per column and per row than forming the difference afterwards.
  // (cs: the step's three battery costs in registers -- BandTune::reads_ahead; a constant after inlining)
  auto ktr_c = [&](int s, const double (&vr)[NR], double vprev, double (&out)[NC], const double* cs = nullptr) {
    out[0] = fma(kd[s][0], vr[1], fma(ks[s][0], vr[0], -(cs ? cs[0] : cof(s, 0))));
    out[1] = fma(kd[s][1], vr[1], fma(ks[s][1], vr[0], -(cs ? cs[1] : cof(s, 1))));
    out[2] = fma(ks[s][2], vr[0], fma(kpv(s), vprev, -(cs ? cs[2] : cof(s, 2))));
    if constexpr (ICE) {
      out[3] = fma(kb[s][0], vr[3], fma(ka[s][0], vr[2], fma(kd[s][3], vr[1], -cof(s, 3))));
      out[4] = fma(kb[s][1], vr[3], fma(ka[s][1], vr[2], -cof(s, 4)));
    }
  };
  auto kown_q = [&](int s, const double (&v)[NC], double (&os)[NR]) {
    os[0] = fma(ks[s][2], v[2], fma(ks[s][1], v[1], fma(ks[s][0], v[0], -qv(s, 0))));
    os[1] = fma(kd[s][1], v[1], fma(kd[s][0], v[0], -qv(s, 1)));
    if constexpr (ICE) {
      os[1] = fma(kd[s][3], v[3], os[1]);
      os[2] = fma(ka[s][1], v[4], fma(ka[s][0], v[3], -rhs(s, 2)));
      os[3] = fma(kb[s][1], v[4], fma(kb[s][0], v[3], -rhs(s, 3)));
    }
  };
  // per-lane partial K'y of the tau columns from the DCM rows' values vd[s] (steps summed in order)
  auto tau_parts = [&](const double (&vd)[S]) {
    if (J == 1) {
      double a = kd[0][2] * vd[0];
#pragma unroll
      for (int s = 1; s < S; ++s) a = fma(kd[s][2], vd[s], a);
      TP[tid] = a;
    } else {
      for (int j = 0; j < J; ++j) {
        double a = (jt[0] == j ? kd[0][2] : 0.0) * vd[0];
#pragma unroll
        for (int s = 1; s < S; ++s) a = fma(jt[s] == j ? kd[s][2] : 0.0, vd[s], a);
        TP[j * B + tid] = a;
      }
    }
  };
  auto tau_parts_of = [&](const double (&vr)[S][NR]) {
    double vd[S];
#pragma unroll
    for (int s = 0; s < S; ++s) vd[s] = vr[s][1];
    tau_parts(vd);
  };
  // wave 0: lane j < J gets the sum over all lanes of TP[j][.] (fixed order; uniform per column)
  auto tau_kt = [&]() {
    double res = 0.0;
    for (int j = 0; j < J; ++j) {
      double a = 0.0;
#pragma unroll
      for (int r = 0; r < NW; ++r) a += TP[j * B + r * kWave + lane];
      a = uniform(wave_sum_dpp(a));
      if (lane == j) res = a;
    }
    return res;
  };

  // ---- ||Kt||_2 by power iteration (as the ELL kernel: v <- Kt'(Kt v), sigma^2 = |v_P| / |v_{P-1}|)
  double eta = o.step_safety;  // Pock-Chambolle bound ||K~|| <= 1, refined by the power iteration
  if (o.power_iters > 0) {
    const int P = o.power_iters;
    const double v0 = 1.0 / sqrt((double)n);
    double vc[S][NC];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int v = 0; v < NC; ++v) vc[s][v] = val[s] ? v0 : 0.0;
    double vtau = (wid == 0 && lane < J) ? v0 : 0.0;
    double nv[2] = {0.0, 0.0};
    double wr[S][NR];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int r = 0; r < NR; ++r) wr[s][r] = 0.0;
    for (int pi = 0; pi <= P; ++pi) {
      if (pi > 0) {
        const double ysp = YS[tid];
#pragma unroll
        for (int s = 0; s < S; ++s) ktr(s, wr[s], s == 0 ? ysp : wr[s > 0 ? s - 1 : 0][0], vc[s]);
        if (wid == 0) {
          const double kt = tau_kt();
          vtau = lane < J ? kt : 0.0;
        }
      }
      if (pi >= P - 1) {
        double a = vtau * vtau;
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int v = 0; v < NC; ++v) a = fma(vc[s][v], vc[s][v], a);
        nv[pi - (P - 1)] = a;
      }
      if (pi == P) break;
      XE[tid] = vc[0][2];
      if (wid == 0 && lane < J) XT[lane] = vtau;
      __syncthreads();
      const double xen = XE[tid + 1];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        kown(s, vc[s], wr[s]);
        kfin_next(s, wr[s], s == S - 1 ? xen : vc[s < S - 1 ? s + 1 : s][2]);
        kfin_tau(s, wr[s]);
      }
      YS[tid + 1] = wr[S - 1][0];
      if (ilane) YS[0] = sp[4] * XE[0];
      tau_parts_of(wr);
      __syncthreads();
    }
    block_sum<B, 2>(nv, red);
    if (nv[0] > 0.0 && nv[1] > 0.0) eta = o.step_safety / sqrt(sqrt(nv[1] / nv[0]));
    YS[tid] = 0.0;
    if (tid == 0) YS[B] = 0.0;
    for (int u = tid; u < kJMax * B; u += B) TP[u] = 0.0;
    __syncthreads();
  }
  if (o.warm) {  // y images of the starting point
    YS[tid + 1] = y[S - 1][0];
    if (ilane) YS[0] = sp[0];
    if (J > 0) tau_parts_of(y);
    __syncthreads();
  }
  eta = uniform(eta);
  // A warm start's primal weight: the geometric mean of the data's (||c~|| / ||q~||) and the starting point's own
  // ||y~0|| / ||x~0|| (PDLP's weight is a ratio of dual to primal movement; the start carries the seed's balance).
  // Bench: PDHG 524.5 -> 520.2 ms per step, warm iterations 2,037.5 -> 2,035.5 (profiles/r03q_ab_warm_pw.log); the
  // start's ratio alone: 523.9 ms.
  double pwi = pw0;
  if (o.warm) {
    double nv[2] = {0.0, 0.0};
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int v = 0; v < NC; ++v) nv[0] += x[s][v] * x[s][v];
#pragma unroll
      for (int r = 0; r < NR; ++r) nv[1] += y[s][r] * y[s][r];
    }
    if (tlane) nv[0] += sp[0] * sp[0];
    if (ilane) nv[1] += sp[0] * sp[0];
    block_sum<B, 2>(nv, red);
    if (nv[0] > 1e-20 && nv[1] > 1e-20) {
      const double ratio = sqrt(nv[1] / nv[0]);
      pwi = sqrt(ratio * pw0);
    }
  }
  double pw = uniform(pwi);
  // ---- box form: x' = (x - lo) / w on the ch / dis / ene columns (after the scaling, the power iteration and the
  //      warm start's weight, which all see the original variables)
  double tj[S][3];  // per-column primal steps tau / w^2 of ch / dis / ene (elec / on: in RO, over their upper bounds)
  double cbox = 0.0;  // c lo, the objective's constant under the change of variables
  if constexpr (BOX) {
    double wb[S][NC];
    bool unb = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int v = 0; v < NC; ++v) {
        double wv = hib(s, v) - (v == 2 ? loe[s] : 0.0);  // padding steps: 0
        unb |= !isfinite(wv);
        if (!(wv >= 0x1p-500)) wv = 0.0;  // a (numerically) fixed column: x' = 0, x = lo
        wb[s][v] = wv;
      }
    }
    if (__syncthreads_or(unb)) {
      bail_plain();
      return;
    }
    // the next lane's first ene (width, lower bound) for the lane's last SOE row; step 0's for the init row
    XP[tid] = wb[0][2];
    XP[B + 1 + tid] = loe[0];
    if (tid == 0) XP[B] = XP[2 * B + 1] = 0.0;
    __syncthreads();
    const double wnx = XP[tid + 1], lnx = XP[B + 2 + tid], we0 = XP[0], le0 = XP[B + 1];
    __syncthreads();  // (XP is rewritten with the images below)
    double cl[1] = {0.0};
    kp0 *= wb[0][2];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double wn1 = s < S - 1 ? wb[s < S - 1 ? s + 1 : s][2] : wnx;
      const double ln1 = s < S - 1 ? loe[s < S - 1 ? s + 1 : s] : lnx;
      if (val[s]) {  // q' = q - K lo over the SOE row: its ene_t and ene_{t+1} terms (ch / dis have lo = 0)
        const double qs = fma(-ks[s][3], ln1, fma(-ks[s][2], loe[s], qv(s, 0)));
        if (LC)
          cqa(3, s) = qs;
        else
          q[s][0] = qs;
        cl[0] = fma(cof(s, 2), loe[s], cl[0]);
      }
      ks[s][0] *= wb[s][0];
      ks[s][1] *= wb[s][1];
      ks[s][2] *= wb[s][2];
      ks[s][3] *= wn1;
      kd[s][0] *= wb[s][0];
      kd[s][1] *= wb[s][1];
      if constexpr (ICE) {  // elec / on: the DCM row's elec term, the two ICE rows (their q: lo = 0, unchanged)
        const double we = wb[s][NC > 3 ? 3 : 0], wo = wb[s][NC > 4 ? 4 : 0];
        kd[s][3] *= we;
        ka[s][0] *= we;
        ka[s][1] *= wo;
        kb[s][0] *= we;
        kb[s][1] *= wo;
      }
#pragma unroll
      for (int v = 0; v < NC; ++v) {
        const double lo = v == 2 ? loe[s] : 0.0, wv = wb[s][v], cs = cof(s, v) * wv;
        if (v >= 3)
          ro(v - 3, s) = cs;
        else if (LC)
          cqa(v, s) = cs;
        else
          cc[s][v] = cs;
        const double xv = wv > 0.0 ? fmin(fmax((x[s][v] - lo) / wv, 0.0), 1.0) : 0.0;
        x[s][v] = xa[s][v] = xv;
        xpi(v, s) = xv;
        if (v < 3)  // the steps tau / w^2
          tj[s][v < 3 ? v : 0] = wv > 0.0 ? uniform(eta / pw) / (wv * wv) : 0.0;
        else
          ro(v - 1, s) = wv > 0.0 ? uniform(eta / pw) / (wv * wv) : 0.0;
      }
    }
    if (ilane) {
      sp[3] = fma(-sp[4], le0, sp[3]);
      sp[4] *= we0;
    }
    block_sum<B, 1>(cl, red);
    cbox = cl[0];
  }
  const double cnorm = uniform(sqrt(nrm[2])), qnorm = uniform(sqrt(nrm[3])), c0 = uniform(b.c0[k] + cbox);
  int it = 0, kin = 0, status = kIterLimit;
  double r0 = -1.0, rprev = -1.0;
  double* fin = red + kNRed * NW;
  if (tid == 0)
    for (int u = 0; u < 4; ++u) fin[u] = NAN;
  const int chk = o.check_every > 0 ? o.check_every : 64;
  double tau = uniform(eta / pw), sigma = uniform(eta * pw);
  double sigma2n = uniform(-2.0 * sigma);  // the equality rows' fused dual step (non-check iterations)
  double tau_bs = tau;                     // (box form) the tau the box steps were last formed for
  // the steps for a new tau from the current ones: tau / w^2 = (tau / tau_bs) (tau_bs / w^2)
  auto box_steps_rescale = [&]() {
    if constexpr (BOX) {
      const double f = uniform(tau / tau_bs);
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int v = 0; v < NC; ++v) {
          if (v < 3)
            tj[s][v < 3 ? v : 0] *= f;
          else
            ro(v - 1, s) *= f;
        }
      tau_bs = tau;
    }
  };
  const int kkt_every = o.kkt_every > 0 ? o.kkt_every : 1;
  int ck = chk, kk_ = kkt_every;
  KktGate gate;  // dvh_options.kkt_predict (dvh_device.h)
  int kbase = 0;
  // The Halpern weights 1 / (k + 2) of the next kWave iterations, one correctly rounded quotient per lane.  (Loaded
  // from a table they sat on the restart path: a restart resets k to 0 and the very next iteration reads weight 0.)
  auto hload = [&](int k0_) { return 1.0 / (k0_ + lane + 2.0); };
  double hw = hload(0);

  // wave 0 with one tau column: the tau reduction is interleaved with its own column work (straight-line code,
  // the partial loads are issued first); J >= 2 takes the generic per-column loop
  const bool w0 = wid == 0 && J == 1;
  double mv0, mv1, mv2, mv3;
  double mvb0 = 0.0, mvb1 = 0.0;  // (box form) the box columns' movements, d'^2 / step
  auto tau_update = [&](double kt, double ca, double cb, auto chk_tag) __attribute__((always_inline)) {
    constexpr bool CHECK = decltype(chk_tag)::value;
    if (tlane) {
      const double xo = sp[0], xan = sp[1];
      const double p1 = vmin(vmax(fma(-tau, sp[2] - kt, xo), sp[3]), sp[4]);
      const double xbt = fma(2.0, p1, -xo);
      XT[lane] = xbt;
      sp[0] = fma(ca, xbt, cb * xan);
      if (CHECK) {
        const double d = xo - p1, da = p1 - xan;
        mv0 += d * d;
        mv1 += da * da;
        sp[5] = p1;
      }
    }
  };
  // the last check iteration's T(z_k) (scaled), from XP / YP
  auto load_images = [&](double (&xp)[S][NC], double (&yp)[S][NR]) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int v = 0; v < NC; ++v) xp[s][v] = xpi(v, s);
#pragma unroll
      for (int r = 0; r < NR; ++r) yp[s][r] = ypi(r, s);
    }
  };
  // (DVH_BAND_PROBE) stamps label the segment they end; a segment is added at the NEXT stamp, so that no stamp waits
  // for its own s_memtime (a stamp's value is first used after the barrier that follows it)
  constexpr int kProbeSegs = 8;
  unsigned pacc[kProbeSegs] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  unsigned long long pt1 = 0ull, pt2 = 0ull;
  auto pstamp = [&](int seg) __attribute__((always_inline)) {
    if constexpr (DVH_BAND_PROBE) {
      const unsigned long long t = probe_clock();
      if (seg < 0) {
        pt1 = pt2 = t;
      } else {
        pacc[(seg + kProbeSegs - 1) % kProbeSegs] += (unsigned)(pt1 - pt2);
        pt2 = pt1;
        pt1 = t;
      }
    }
  };
  // (Tune::reads_ahead) the reads carried from one plain iteration to the next (BandAhead).  iterate takes the object as
  // an argument and keeps no local of its own for this: one more capture of that lambda, a local array in it or a
  // generic ktr_c each changed the register allocation of the forms that do not use any of it.
  using F = std::integral_constant<bool, false>;
  using Tt = std::integral_constant<bool, true>;
  std::conditional_t<Tune::reads_ahead, BandAhead<B, S>, BandNoAhead> ah;
  if constexpr (Tune::reads_ahead) {
    ah.tp = TP + lane;
    ah.ys = YS + tid;
    ah.cq = CQ + tid;
  }
  auto iterate = [&](auto chk_tag, auto w0_tag, auto& ahd) __attribute__((always_inline)) {
    constexpr bool CHECK = decltype(chk_tag)::value;
    constexpr bool W0 = decltype(w0_tag)::value;
    constexpr bool RA = !CHECK && Tune::reads_ahead;
    constexpr bool LATE = !W0 || (!CHECK && Tune::w0_late);
    if constexpr (W0) __builtin_amdgcn_s_setprio(kTauWavePrio);  // until the first barrier
    pstamp(7);  // (the check code since the last iteration, or the loop entry)
    if (kin - kbase >= kWave) {
      kbase = kin;
      hw = hload(kin);
    }
    const double cb = readlane_f64(hw, kin - kbase), ca = 1.0 - cb;
    mv0 = mv1 = mv2 = mv3 = 0.0;
    mvb0 = mvb1 = 0.0;
    // ---------------- primal half-step (reflected Halpern, rho = 1)
    double kx[S][NR];  // own-lane part of K x-bar for the dual half-step
    // the dual update of step s's r-th row from kx (row 0, SOE, is an equality; DCM / ICE rows are >=: duals >= 0)
    auto row_step = [&](int s, int r) __attribute__((always_inline)) {
      if (!CHECK && r == 0) {  // equality row, no image needed: 2 (y - sigma Kx) - y = y - 2 sigma Kx
        y[s][0] = fma(ca, fma(sigma2n, kx[s][0], y[s][0]), cb * ya[s][0]);
        return;
      }
      double p1 = fma(-sigma, kx[s][r], y[s][r]);
      if (r > 0) p1 = vmax(p1, 0.0);
      if (CHECK) {
        const double d = y[s][r] - p1, da = p1 - ya[s][r];
        mv2 += d * d;
        mv3 += da * da;
        ypi(r, s) = p1;
      }
      y[s][r] = fma(ca, fma(2.0, p1, -y[s][r]), cb * ya[s][r]);
    };
    {
      double ta0 = 0.0, ta1 = 0.0;
      if constexpr (W0 && RA) {  // (the partials read behind the last second barrier, summed in the same order)
        ta0 = ahd.t[0];
        if (NW > 1) ta1 = ahd.t[1];
#pragma unroll
        for (int r = 2; r < NW; r += 2) {
          ta0 += ahd.t[r];
          if (r + 1 < NW) ta1 += ahd.t[r + 1];
        }
      } else if constexpr (W0) {  // (0 + a == a: the first partials start the two chains)
        ta0 = TP[lane];
        if (NW > 1) ta1 = TP[kWave + lane];
#pragma unroll
        for (int r = 2; r < NW; r += 2) {
          ta0 += TP[r * kWave + lane];
          if (r + 1 < NW) ta1 += TP[(r + 1) * kWave + lane];
        }
      }
      double kty[S][NC], xb[S][NC];
      if constexpr (RA) {
#pragma unroll
        for (int s = 0; s < S; ++s) ktr_c(s, y[s], s == 0 ? ahd.y : y[s > 0 ? s - 1 : 0][0], kty[s], ahd.c[s]);
      } else {
        const double ysp = YS[tid];
#pragma unroll
        for (int s = 0; s < S; ++s) ktr_c(s, y[s], s == 0 ? ysp : y[s > 0 ? s - 1 : 0][0], kty[s]);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int v = 0; v < NC; ++v) {  // branch-free: padding steps have c = lo = hi = 0 and stay at 0
          double p1;
          if constexpr (BOX) {
            p1 = fma_clamp01(v < 3 ? tj[s][v < 3 ? v : 0] : ro(v - 1, s), kty[s][v], x[s][v]);
          } else {
            const double lo = v == 2 ? loe[s] : 0.0;
            p1 = vmin(vmax(fma(tau, kty[s][v], x[s][v]), lo), hib(s, v));
          }
          xb[s][v] = fma(2.0, p1, -x[s][v]);
          if (CHECK) {
            double d = x[s][v] - p1, da = p1 - xa[s][v];
            if constexpr (BOX) {  // movements in x units: w^2 = tau_bs / step (0 for a fixed column)
              const double st = v < 3 ? tj[s][v < 3 ? v : 0] : ro(v - 1, s);
              const double iw = st > 0.0 ? (double)__builtin_amdgcn_rcp(st) : 0.0;
              mvb0 = fma(d * d, iw, mvb0);
              mvb1 = fma(da * da, iw, mvb1);
            } else {
              mv0 += d * d;
              mv1 += da * da;
            }
            xpi(v, s) = p1;
          }
          if constexpr (RA)
            ahd.xb[s][v] = xb[s][v];
          else
            x[s][v] = fma(ca, xb[s][v], cb * xa[s][v]);
        }
      }
      XE[tid] = xb[0][2];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        kown_q(s, xb[s], kx[s]);
        if (s < S - 1) kfin_next(s, kx[s], xb[s < S - 1 ? s + 1 : s][2]);  // the next step is the lane's own
      }
      if constexpr (W0) {
        tau_update(uniform(wave_sum_dpp(ta0 + ta1)), ca, cb, chk_tag);
      } else {
        if (wid == 0 && J > 1) tau_update(tau_kt(), ca, cb, chk_tag);
      }
    }
    pstamp(0);
    if constexpr (!W0 && Tune::pin_kx) {  // K x-bar before the barrier: the compiler sank it into the dual half-step
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int r = 0; r < NR; ++r) asm volatile("" ::"v"(kx[s][r]));
    }
    lds_barrier();
    // every LDS read of the dual half-step together (the next lane's ene, the tau columns' x-bar), before any LDS
    // store: one wait instead of one per read
    double xen, xtv[S], xe0 = 0.0;
    auto dual_reads = [&]() __attribute__((always_inline)) {
      xen = XE[tid + 1];
      if constexpr (J1) {  // one tau column: one read
        const double xt0 = XT[0];
#pragma unroll
        for (int s = 0; s < S; ++s) xtv[s] = xt0;
      } else {
#pragma unroll
        for (int s = 0; s < S; ++s) xtv[s] = lds_ld(xta[s]);
      }
    };
    // (Tune::w0_reads_first) wave 0 issues them in front of the priority drop, and the init row's ene_0 (lane kInitLane;
    // a broadcast read) with them: s_setprio is a scheduling boundary, so the reads behind it started after the x-bar and
    // K x-bar work the compiler sinks across the barrier and were waited for at once; in front of it that work runs under
    // their latency, and the init row's block at the end of the half-step has nothing left to wait for
    constexpr bool RF = W0 && Tune::w0_reads_first;
    if constexpr (RF) {
      dual_reads();
      xe0 = XE[0];
    }
    if constexpr (W0) __builtin_amdgcn_s_setprio(0);
    pstamp(1);
    // ---------------- dual half-step
    {
      if constexpr (!RF) dual_reads();
      kfin_next(S - 1, kx[S - 1], xen);
      // the >= rows first: their duals feed the tau partials, whose wave reduction then has the SOE rows' work
      // beside it
#pragma unroll
      for (int s = 0; s < S; ++s) {
        kx[s][1] = fma(kd[s][2], xtv[s], kx[s][1]);  // kfin_tau
#pragma unroll
        for (int r = 1; r < ((ICE && !W0) ? 2 : NR); ++r) row_step(s, r);  // (the ICE rows: see below)
      }
      if (J > 0) tau_parts_of(y);
#pragma unroll
      for (int s = LATE ? S - 1 : 0; s < S; ++s) row_step(s, 0);  // (the lane-local SOE rows: see below)
      YS[tid + 1] = y[S - 1][0];
      pstamp(2);
      if (W0 || (!J1 && wid == 0)) {  // init row (lane kInitLane): ene_0 = target; (J1: wave 0 is always W0)
        if (ilane) {
          const double y0 = sp[0], ya0 = sp[1];
          const double q1 = fma(sigma, sp[3] - sp[4] * (RF ? xe0 : XE[0]), y0);
          if (CHECK) {
            const double d = y0 - q1, da = q1 - ya0;
            mv2 += d * d;
            mv3 += da * da;
            sp[2] = q1;
          }
          const double yn = fma(ca, fma(2.0, q1, -y0), cb * ya0);
          sp[0] = yn;
          YS[0] = yn;
        }
      }
    }
    ++it;
    ++kin;
    pstamp(3);
    // Wave 0's check iteration finishes its Halpern blends (x = ca x-bar + cb x-anchor, and the rows') before the second
    // barrier.  The plain iteration did so too (profiles/r06j_pin_blend.log, when wave 0 waited for the others at that
    // barrier); since Tune::w0_reads_first it is the wave the others wait for there, and with Tune::w0_late its plain
    // iteration leaves the blends to the far side of the barrier, as the other waves do.
    if constexpr (W0 && !LATE) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int v = 0; v < NC; ++v) asm volatile("" ::"v"(x[s][v]));
#pragma unroll
        for (int r = 0; r < NR; ++r) asm volatile("" ::"v"(y[s][r]));
      }
    }
    pstamp(4);
    lds_barrier();
    pstamp(5);  // (directly behind the barrier: the wait alone, without the late rows)
    // The waves without the tau column update the SOE rows of their lanes' steps 0 .. S - 2, and the two ICE rows, after
    // the barrier instead of before it (those duals are read only by the lane's own next primal half-step), so that they
    // reach the barrier -- which wave 0's next tau reduction waits behind -- sooner (profiles/r06s_ab.log,
    // r06m_late_ice.log).  With Tune::w0_late wave 0's plain iteration does the same: it is the wave the others wait for at
    // this barrier.
    // (Tune::reads_ahead) the next primal half-step's reads first, then -- nothing crosses the sched_barrier, without it
    // the scheduler issued the reads behind the blends and waited for them at once -- the x blends, placed here in the
    // source, and the late rows under the reads' latency; hold_ahead ends the block.  No barrier, branch or lane mask
    // is involved: reads, lane-local arithmetic and two scheduling directives.
    if constexpr (RA) {
      ahd.template read<W0>();
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int v = 0; v < NC; ++v) x[s][v] = fma(ca, ahd.xb[s][v], cb * xa[s][v]);
    }
    if constexpr (LATE) {
#pragma unroll
      for (int s = 0; s < S - 1; ++s) row_step(s, 0);
    }
    if constexpr (ICE && !W0) {
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int r = 2; r < NR; ++r) row_step(s, r);
    }
    if constexpr (RA) ahd.template hold<W0>();
    pstamp(6);
  };

  pstamp(-1);
  // The plain iterations between two checks run in an innermost loop of their own, one per wave kind
  // (Tune::plain_loop).  As `if (--ck != 0) { iterate; continue; }` in this loop, the plain iteration was a branch of
  // the one region LLVM makes of the loop over windows and this loop: every iteration left it through a chain of about
  // ten flag-driven scalar branches and a block of 17 v_mov_b64 that copied the new x, y, tau and init-row values back
  // to the registers the next iteration reads (the phis were not coalesced), at the head of wave 0's primal half-step.
  // The inner loops keep those values in place (scripts/loop_shape.py, profiles/band_loop_shape.txt).
  // Same iterations, same checks: ck - 1 plain iterations precede the check at ck = 1, fewer where max_iters comes first
  // (the loop then ends without a check, as before); it, kin and ck end up as the one-by-one form leaves them.
  // Barriers: np comes from ck, o.max_iters and it, which are the same in every wave of the workgroup (kernel arguments
  // and counters every wave advances alike), so every wave runs the same number of trips, the exit is a scalar branch
  // on an SGPR counter, and both loop bodies pass the iteration's two barriers once per trip on every path (what differs
  // between the two, and what their lane masks skip, holds no barrier) -- the waves of a workgroup, some in one loop and
  // some in the other, meet at every barrier.  (The two traps of the persistent loop below apply here as well: a
  // lane-dependent trip count would be structurized into a loop whose barriers the waves do not reach in step.)
  // The single-demand-period instantiation (J1) keeps all of this: it adds no loop and changes no trip count (np is formed
  // as before), w0 is then wid == 0, a scalar, so each wave still takes one of the same two loops, and what J1 takes
  // out of the other waves' body -- the J > 1 tau update, the init row, the per-step XT reads -- are lane-masked blocks
  // and LDS reads without a barrier: both bodies still pass both barriers once per trip, and the other waves' body
  // becomes an innermost loop without the two child loops over the tau columns (profiles/band_j1_shape.txt).
  // Tune::w0_reads_first moves LDS reads of wave 0's body to the other side of an s_setprio and adds one broadcast read:
  // no barrier, no branch and no lane mask is added or moved (profiles/band_w0_shape.txt).
  // Tune::w0_late and Tune::reads_ahead keep all of this as well.  The first moves lane-local row updates and blends of
  // wave 0's body from one side of the second barrier to the other.  The second adds LDS reads in front of each loop
  // (straight-line, every lane, no barrier) and moves the body's reads of YS, TP and the costs from its head to its
  // tail, behind the second barrier of the same trip: between that barrier and the next trip's first barrier nothing
  // writes YS or TP, so the carried values are what the head would have read, on every trip including the first; the
  // trip that leaves the loop reads once for nothing.  np, the exit branch and both barriers are untouched, so both
  // bodies still pass both barriers once per trip on every path (profiles/band_reads_shape.txt), and the two traps
  // named above apply unchanged: nothing here depends on the lane.
  while (it < o.max_iters) {
    if constexpr (Tune::plain_loop) {
      if (ck > 1) {  // the ck - 1 plain iterations up to the next check, or those left to max_iters
        int np = min(ck - 1, o.max_iters - it);
        ck -= np;
        if (w0) {
          if constexpr (Tune::reads_ahead) ah.template read<true>();
          do iterate(F(), Tt(), ah);
          while (--np != 0);
        } else {
          if constexpr (Tune::reads_ahead) ah.template read<false>();
          do iterate(F(), F(), ah);
          while (--np != 0);
        }
        continue;
      }
    } else if (--ck != 0) {
      if (w0)
        iterate(F(), Tt(), ah);
      else
        iterate(F(), F(), ah);
      continue;
    }
    ck = chk;
    if (w0)
      iterate(Tt(), Tt(), ah);
    else
      iterate(Tt(), F(), ah);
    // ---------------- check: fixed-point residual of z_k, restart test; every kkt_every-th check the relative
    // KKT error of T(z_k) in the unscaled space (as pdhg_ell_kernel)
    const bool last = it + chk > o.max_iters;
    bool kkt = (--kk_ == 0) || last;
    if (kkt) kk_ = kkt_every;
    static_assert(kRdx == kNRed - 1, "the dual-residual term is the last reduced value");
    constexpr int NRED = Tune::gate_rdx ? kNRed : kNRed - 1;
    double acc[NRED];
    acc[0] = fma(tau_bs, mvb0, mv0);  // (mvb0 = mvb1 = 0 in the plain form)
    acc[1] = fma(tau_bs, mvb1, mv1);
    acc[2] = mv2;
    acc[3] = mv3;
#pragma unroll
    for (int u = 4; u < NRED; ++u) acc[u] = 0.0;
    double r = 0.0;
    if constexpr (GATE) {
      // predicted KKT gate: the restart sums first; a due check runs only if the last check's worst ratio to eps,
      // scaled by the fixed-point residual's decrease since then, is within kkt_predict (or 4 were skipped)
      double acc4[4] = {acc[0], acc[1], acc[2], acc[3]};
      block_sum1<B, 4, true>(acc4, red);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = acc4[u];
      r = usc<USC>(sqrt(pw * acc[0] + acc[2] / pw));
      if (kkt && !last && kkt_gate_skip(o, gate, r)) {
        kkt = false;
        ++gate.skip;
      }
    }
    if (kkt) {
      // (Tune::kkt_prefetch) the single-precision factors of the lane's columns and rows, loaded together first: one wait
      // for all of them, behind the image reads and the barrier below
      // (branch-free: a padding step / absent row loads the window's first entry and discards it; the indices are
      // formed here from an opaque thread index, so that they are not hoisted out of the loop and held)
      float fcl[S][NC], frl[S][NR], fspl = 1.0f;
      if constexpr (Tune::kkt_prefetch) {
        const int to = S * opaque(tid);
        const float* fcw = w.fc + W.wn;
        const float* frw = w.fr + W.wm;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const bool vs = to + s < T;
#pragma unroll
          for (int v = 0; v < NC; ++v) {
            const int j = v < 3 ? v * T + to + s : (v == 3 ? CE : CO) + to + s;
            const float f = fcw[vs ? j : 0];
            fcl[s][v] = vs ? f : 1.0f;
          }
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const int i = r == 0 ? (vs ? to + s + 1 : -1) : r == 1 ? DRL[s * B + tid] : (vs ? (r == 2 ? ra[s] : rb[s]) : -1);
            const float f = frw[i >= 0 ? i : 0];
            frl[s][r] = i >= 0 ? f : 1.0f;
          }
        }
        const int lo_ = (to / S) & (kWave - 1);  // (the lane, from the opaque thread index)
        const float ft = fcw[tlane ? 3 * T + lo_ : 0], fi = frw[0];
        fspl = tlane ? ft : ilane ? fi : 1.0f;
      }
      // images of T(z_k) in XE / XT / YS / TP (rewritten from z after the check)
      double xp[S][NC], yp[S][NR];
      load_images(xp, yp);
      XE[tid] = xp[0][2];
      YS[tid + 1] = yp[S - 1][0];
      if (ilane) YS[0] = sp[2];
      if (tlane) XT[lane] = sp[5];
      if (J > 0) tau_parts_of(yp);
      lds_barrier();
      auto col_kkt = [&](int j, double kt, double cj, double loj, double hij, double xj, float fpre) {
        const float fd = Tune::kkt_prefetch ? fpre : w.fc[W.wn + opaque(j)];
        static_assert(Tune::gate_rdx == Tune::kkt_inline, "col_kkt_x_i is inlined only, col_kkt_o out of line only");
        if constexpr (Tune::gate_rdx) {
          const ColKktX r = col_kkt_x_i(kt, cj, loj, hij, xj, fd);
          acc[5] += r.rd2;
          acc[6] += r.cx;
          acc[8] += r.bt;
          acc[kRdx] += r.rdx;
        } else {
          const ColKkt r = col_kkt_o(kt, cj, loj, hij, xj, fd);
          acc[5] += r.rd2;
          acc[6] += r.cx;
          acc[8] += r.bt;
        }
      };
      auto row_kkt = [&](int i, double kv, double qi, double yi, bool ge, float fpre) {
        const float fd = Tune::kkt_prefetch ? fpre : w.fr[W.wm + opaque(i)];
        const RowKkt r = row_kkt_fn<Tune::kkt_inline>(kv, qi, yi, fd, ge);
        acc[4] += r.rp2;
        acc[7] += qi * yi;
        acc[9] += r.y2;
      };
      const double ysp = YS[tid];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        double kt[NC];
        ktr(s, yp[s], s == 0 ? ysp : yp[s > 0 ? s - 1 : 0][0], kt);
        if (val[s]) {
#pragma unroll
          for (int v = 0; v < NC; ++v) {
            if constexpr (BOX)  // the primed LP: box [0, 1]
              col_kkt(col(s, v), kt[v], cof(s, v), 0.0, 1.0, xp[s][v], fcl[s][v]);
            else
              col_kkt(col(s, v), kt[v], cof(s, v), v == 2 ? loe[s] : 0.0, hib(s, v), xp[s][v], fcl[s][v]);
          }
        }
      }
      if (wid == 0 && J > 0) {
        const double ktt = tau_kt();
        if (tlane) col_kkt(3 * T + lane, ktt, sp[2], sp[3], sp[4], sp[5], fspl);
      }
      const double xen = XE[tid + 1];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        double kv[NR];
        kown(s, xp[s], kv);
        kfin_next(s, kv, s == S - 1 ? xen : xp[s < S - 1 ? s + 1 : s][2]);
        kfin_tau(s, kv);
        const int t = t0 + s;
        if (val[s]) row_kkt(t + 1, kv[0], qv(s, 0), yp[s][0], false, frl[s][0]);
        const int dr_ = DRL[s * B + tid];
        if (dr_ >= 0) row_kkt(dr_, kv[1], qv(s, 1), yp[s][1], true, frl[s][1]);
        if (ICE && val[s]) {
          row_kkt(ra[s], kv[2], rhs(s, 2), yp[s][2], true, frl[s][NR > 2 ? 2 : 0]);
          row_kkt(rb[s], kv[3], rhs(s, 3), yp[s][3], true, frl[s][NR > 3 ? 3 : 0]);
        }
      }
      if (ilane) row_kkt(0, sp[4] * XE[0], sp[3], sp[2], false, fspl);
    }
    if constexpr (GATE) {
      if (kkt) {  // the KKT sums in the slots after the restart sums' (red is not reused before a barrier)
        double acc6[NRED - 4];
#pragma unroll
        for (int u = 4; u < NRED; ++u) acc6[u - 4] = acc[u];
        block_sum1<B, NRED - 4, true>(acc6, red + 4 * NW);
#pragma unroll
        for (int u = 4; u < NRED; ++u) acc[u] = acc6[u - 4];
      }
    } else if (kkt) {
      block_sum1<B, NRED, true>(acc, red);
    } else {
      double acc4[4] = {acc[0], acc[1], acc[2], acc[3]};
      block_sum1<B, 4, true>(acc4, red);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = acc4[u];
    }
    if constexpr (!GATE) r = usc<USC>(sqrt(pw * acc[0] + acc[2] / pw));
    if (kkt) {
      const double pobj = usc<USC>(acc[6] + c0), dobj = usc<USC>(acc[7] + acc[8] + c0);
      const double pres = usc<USC>(sqrt(acc[4]) / (1.0 + sgpr_fresh<USC>(qnorm)));
      const double dres = usc<USC>(sqrt(acc[5]) / (1.0 + sgpr_fresh<USC>(cnorm)));
      const double gap = usc<USC>(fabs(pobj - dobj) / (1.0 + fabs(pobj) + fabs(dobj)));
      if (tid == 0) {
        fin[0] = pobj;
        fin[1] = pres;
        fin[2] = dres;
        fin[3] = gap;
      }
      if (kkt_done(o, pres, dres, gap, pobj, dobj, acc[4], acc[9], Tune::gate_rdx ? acc[kRdx] : 0.0)) {
        status = kOptimal;
        break;
      }
      if constexpr (GATE) {
        gate.note(pres, dres, gap, o.eps, r);
        gate.q = usc<USC>(gate.q);
      }
      if (!(isfinite(pobj) && isfinite(dobj))) {
        status = kNumerical;
        break;
      }
    }
    if (r0 < 0.0) r0 = r;
    const bool restart = (r <= o.b_suff * r0) || (r <= o.b_nec * r0 && rprev >= 0.0 && r > rprev) ||
                         ((double)kin >= o.b_art * (double)it);
    if (restart) {
      const double ddx = sqrt(acc[1]), ddy = sqrt(acc[3]);
      if (ddx > 1e-10 && ddy > 1e-10) pw = uniform(pw_update<!ICE>(ddy / ddx, pw, o.theta));
      tau = uniform(eta / pw);
      sigma = uniform(eta * pw);
      sigma2n = uniform(-2.0 * sigma);
      box_steps_rescale();
      double xp[S][NC], yp[S][NR];
      load_images(xp, yp);
#pragma unroll
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int v = 0; v < NC; ++v) {
          x[s][v] = xa[s][v] = xp[s][v];
        }
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
          y[s][rr] = ya[s][rr] = yp[s][rr];
        }
      }
      if (ilane) sp[0] = sp[1] = sp[2];
      if (tlane) sp[0] = sp[1] = sp[5];
      kin = 0;
      kbase = 0;
      hw = hload(0);
      r0 = r;
      rprev = -1.0;
    } else {
      rprev = r;
    }
    if (restart || kkt) {  // the y images must hold z again (after a restart z = T(z_k))
      YS[tid + 1] = y[S - 1][0];
      if (ilane) YS[0] = sp[0];
      if (J > 0) tau_parts_of(y);
      lds_barrier();
    }
    // (a restart check that neither restarts nor checks KKT rewrote no shared value: the next iteration reads what the
    // check iteration wrote before its barriers, and `red` is next written two barriers later -- no barrier here)
  }
  // outputs: the last check's T(z_k), unscaled
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (!val[s]) continue;
    const int t = t0 + s;
#pragma unroll
    for (int v = 0; v < NC; ++v) {
      const int j = col(s, v);
      if constexpr (BOX) {  // x = lo + w x' (clipped to the box against the rounding), then unscaled
        const double d = dcf(j), lo = lraw[j] / d, hv = uraw[j] / d;
        double wv = hv - (v == 2 ? lo : 0.0);  // the set-up's width, by the set-up's operations
        if (!(wv >= 0x1p-500)) wv = 0.0;
        xo_g[j] = unscale_x(fmin(fmax(fma(wv, xpi(v, s), lo), lo), hv), d, lraw[j], uraw[j]);
      } else {
        xo_g[j] = unscale_x(xpi(v, s), dcf(j), lraw[j], uraw[j]);
      }
    }
    yo_g[t + 1] = ypi(0, s) * drf(t + 1);
    const int dr_ = DRL[s * B + tid];
    if (dr_ >= 0) yo_g[dr_] = ypi(1, s) * drf(dr_);
    if (ICE) {
      yo_g[ra[s]] = ypi(2, s) * drf(ra[s]);
      yo_g[rb[s]] = ypi(3, s) * drf(rb[s]);
    }
  }
  if (tlane) xo_g[3 * T + lane] = unscale_x(sp[5], dcf(3 * T + lane), lraw[3 * T + lane], uraw[3 * T + lane]);
  if (ilane) yo_g[0] = sp[2] * drf(0);
  if constexpr (DVH_BAND_PROBE) {
    pstamp(kProbeSegs - 1);
    pacc[kProbeSegs - 1] += (unsigned)(pt1 - pt2);
    unsigned hw = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    __syncthreads();
    if (lane == 0) {
      for (int u = 0; u < kProbeSegs; ++u) xo_g[(kProbeSegs + 1) * wid + u] = (double)pacc[u];
      xo_g[(kProbeSegs + 1) * wid + kProbeSegs] = (double)hw;
    }
  }
  if (tid == 0) {
    b.istats[2 * k] = status;
    b.istats[2 * k + 1] = it;
    for (int u = 0; u < 4; ++u) b.stats[4 * k + u] = fin[u];
  }
}

// Persistent form (PERSIST: the three-step battery form and the ICE form): the grid is the device's resident workgroup
// slots, and each workgroup takes the next window from an atomic counter until the list is exhausted, so a slot freed
// by a short window takes the next one at once.  One workgroup per window left the slots to the hardware dispatcher,
// which deals workgroups in order round-robin over the XCDs: with durations that vary window to window (warm
// iterations 200 .. 10,000) the in-order dispatch leaves slots idle (profiles/r04r_ab_launch_order.log,
// r04t_probe_dispatch.log, r04u_ab_band_queue.log, r04an_ab_ice_queue.log).  Every workgroup leaves once the counter
// passes the list (the counter zeroed on the stream before the launch).  The one-step battery form stays one workgroup
// per window.
struct BandArgs {
  Batch b;
  Work w;
  Chunk ch;
  Opts o;
  const int32_t* list;  // global window indices, or null: the chunk
  int count;            // windows to solve (list entries, or the chunk's)
  int32_t* queue;       // work-queue counter (PERSIST), zeroed before the launch
};
template <int B, int S, bool ICE, bool LC, int WPS, bool GATE, bool BOX, bool PERSIST>
__global__ __launch_bounds__(B, WPS) void pdhg_band_kernel(const BandArgs args) {
  if constexpr (!PERSIST) {
    const int i = blockIdx.x;
    band_window<B, S, ICE, LC, WPS, GATE, BOX>(args.b, args.w, args.ch, args.o,
                                               args.list ? args.list[i] : args.ch.first + i, threadIdx.x);
  } else {
    __shared__ int32_t next;
    for (;;) {
#if defined(__HIP_DEVICE_COMPILE__)
      // The arguments are read through a kernarg pointer the compiler cannot see through, once per window: read as
      // `args`, their ~70 scalar loads were hoisted out of this loop and kept live across the window (SGPRs spilled
      // to VGPR lanes, 56 dwords of VGPRs to scratch; 12.6 % slower per iteration than one workgroup per window at
      // equal durations, profiles/r04ak_band_queue_iter.log).  Laundered, each window reloads what it uses.
      using KArgs = const __attribute__((address_space(4))) BandArgs*;
      KArgs kp = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(kp));
      const BandArgs& args = *(const BandArgs*)kp;
#endif
      // wave 0 takes the next window in a wave-uniform branch, the whole wave in the atomic (lane 0 adds 1, the others
      // 0): a lane-0-only atomic inside the loop is structurized into an inner loop whose barriers the waves do not
      // reach in step (the workgroups hang: scripts/probe_dispatch.hip)
      if (__builtin_amdgcn_readfirstlane(threadIdx.x) < kWave)
        next = __builtin_amdgcn_readfirstlane(atomicAdd(args.queue, (threadIdx.x & (kWave - 1)) == 0 ? 1 : 0));
      __syncthreads();
      const int i = __builtin_amdgcn_readfirstlane(next);  // uniform: the loop's exit is a scalar branch
      __syncthreads();  // (every wave has read it before wave 0 takes the next one)
      if (i >= args.count) return;
      int tid = threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+v"(tid));  // (likewise what the window derives from its thread index)
#endif
      band_window<B, S, ICE, LC, WPS, GATE, BOX>(args.b, args.w, args.ch, args.o,
                                                 args.list ? args.list[i] : args.ch.first + i, tid);
    }
  }
}

// The single-demand-period instantiation (band_window, J1) of the persistent form: pdhg_band_kernel's persistent loop
// again, statement for statement (its comments hold here too), in a kernel of its own name and text.  (One body inlined
// into both kernels changed the machine code of every other form, the ICE form's included, and a further template
// parameter their symbols.)
template <int B, int S, bool ICE, bool LC, int WPS, bool GATE, bool BOX>
__global__ __launch_bounds__(B, WPS) void pdhg_band_kernel_j1(const BandArgs args) {
  __shared__ int32_t next;
  for (;;) {
#if defined(__HIP_DEVICE_COMPILE__)
    using KArgs = const __attribute__((address_space(4))) BandArgs*;
    KArgs kp = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    const BandArgs& args = *(const BandArgs*)kp;
#endif
    if (__builtin_amdgcn_readfirstlane(threadIdx.x) < kWave)
      next = __builtin_amdgcn_readfirstlane(atomicAdd(args.queue, (threadIdx.x & (kWave - 1)) == 0 ? 1 : 0));
    __syncthreads();
    const int i = __builtin_amdgcn_readfirstlane(next);
    __syncthreads();
    if (i >= args.count) return;
    int tid = threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(tid));
#endif
    band_window<B, S, ICE, LC, WPS, GATE, BOX, true>(args.b, args.w, args.ch, args.o,
                                                     args.list ? args.list[i] : args.ch.first + i, tid);
  }
}

template <int B, int S, bool ICE, bool LC, int WPS, bool GATE, bool BOX, bool PERSIST>
hipError_t launch_band_one_q(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                             const int32_t* list, int nlist, int* variant_out) {
  static_assert(B * S == kBandSteps, "every form covers T <= kBandSteps");
  const size_t lds = band_lds_bytes(B, S, ICE, LC);
  auto kern = pdhg_band_kernel<B, S, ICE, LC, WPS, GATE, BOX, PERSIST>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  if (getenv("DVH_BAND_OCC")) {  // residency diagnostics (A/B helper)
    int nb = -1, dev = 0;
    hipGetDevice(&dev);
    hipDeviceProp_t pr;
    hipGetDeviceProperties(&pr, dev);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)kern, B, lds);
    hipFuncAttributes fa;
    hipFuncGetAttributes(&fa, (const void*)kern);
    fprintf(stderr, "band<%d,%d,%d,%d,gate %d,box %d,persist %d>: lds %zu B, blocks/CU %d, lds/CU %zu, regs %d, local %zu\n",
            B, S, (int)ICE, (int)LC, (int)GATE, (int)BOX, (int)PERSIST, lds, nb, (size_t)pr.maxSharedMemoryPerMultiProcessor,
            fa.numRegs, (size_t)fa.localSizeBytes);
  }
  const int count = list ? nlist : ch.count;
  if (count <= 0) return hipSuccess;
  int grid = count;
  if (PERSIST) {  // every resident slot (workgroups per CU at this form x CUs), or fewer
    // measured once per handle (each handle belongs to one device and one host thread at a time; Work::slots)
    int& slots = w.slots[(ICE ? 4 : 0) + (GATE ? 2 : 0) + (BOX ? 1 : 0)];
    if (slots <= 0) {
      int nb = 0, cus = 0, dev = 0;
      if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
      if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)kern, B, lds)) != hipSuccess) return e;
      if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
      slots = std::max(1, nb) * std::max(1, cus);
    }
    // DVH_BAND_RESERVE = k: leave 2k workgroup slots to other kernels, e.g. an all-gather issued on another stream
    // after this grid launched, which otherwise waits for the grid's tail (scripts/probe_overlap.py,
    // profiles/r05i_overlap_reserve*.log: k = 32 lets a 2 GiB copy run beside the grid at +12.6 % band time)
    static const int reserve = [] { const char* e = getenv("DVH_BAND_RESERVE"); return e ? std::max(0, atoi(e)) : 0; }();
    grid = std::min(count, std::max(1, slots - 2 * reserve));
    if ((e = hipMemsetAsync(w.queue, 0, sizeof(int32_t), s)) != hipSuccess) return e;
  }
  const BandArgs args{b, w, ch, o, list, count, w.queue};
  hipLaunchKernelGGL(kern, dim3(grid), dim3(B), lds, s, args);
  if (variant_out) *variant_out = 9000000 + 1000 * (S - 1) + (ICE ? 100 : 0) + B / kWave;
  return hipGetLastError();
}
template <int B, int S, bool ICE, bool LC, int WPS, bool GATE, bool BOX>
hipError_t launch_band_one_g(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                             const int32_t* list, int nlist, bool j1, int* variant_out) {
  if constexpr (S == 3 && !ICE) {  // the persistent form (DVH_BAND_QUEUE=0: one workgroup per window, A/B)
    static_assert(B == kBandSteps / 3 && LC && WPS == 2, "dvh_band_persist.hip instantiates this form");
    const char* q = getenv("DVH_BAND_QUEUE");
    if (!(q && atoi(q) == 0)) return launch_band_persist(GATE, BOX, j1, b, w, ch, o, s, list, nlist, variant_out);
  }
  if constexpr (ICE) {  // the ICE form's persistent grid (DVH_BAND_QUEUE=0 or DVH_BAND_QUEUE_ICE=0: off, A/B)
    static_assert(B == kBandSteps && S == 1 && !LC && WPS == 3, "dvh_band_persist_ice.hip instantiates this form");
    const char* q = getenv("DVH_BAND_QUEUE");
    const char* qi = getenv("DVH_BAND_QUEUE_ICE");
    if (!(q && atoi(q) == 0) && !(qi && atoi(qi) == 0))
      return launch_band_persist_ice(GATE, BOX, b, w, ch, o, s, list, nlist, variant_out);
  }
  return launch_band_one_q<B, S, ICE, LC, WPS, GATE, BOX, false>(b, w, ch, o, s, list, nlist, variant_out);
}
template <int B, int S, bool ICE, bool LC, int WPS, bool BOX = false>
hipError_t launch_band_one(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                           const int32_t* list, int nlist, bool j1, int* variant_out) {
  if (o.kkt_predict > 0)
    return launch_band_one_g<B, S, ICE, LC, WPS, true, BOX>(b, w, ch, o, s, list, nlist, j1, variant_out);
  return launch_band_one_g<B, S, ICE, LC, WPS, false, BOX>(b, w, ch, o, s, list, nlist, j1, variant_out);
}

}  // namespace

// The form for a batch (the file header lists them): form 3, the default, is the three-step battery form, form 1 the
// one-step one (dvh_set_kernel_path 3; dvh_api.cpp takes it for batches of at most one window per CU); the LP-relaxed
// ICE windows have the one-step ICE form only.  (A 384-thread, two-step form with 3 waves per SIMD ran one window per
// CU in practice: its 6 waves cannot be placed 3 / 3 / 3 / 3; profiles/r02x_band_forms.log.)
#if DVH_BAND_PERSIST_TU == 1
// The persistent forms (three-step battery: dvh_band_persist.hip, DVH_BAND_PERSIST_TU 1; ICE: dvh_band_persist_ice.hip, 2),
// each this file in a translation unit of its own, compiled without
// machine-level loop-invariant code motion: hoisted out of the persistent loop, the window setup's invariants stayed live
// across every window's iterations (56 spilled dwords, 12.6 % slower per iteration than one workgroup per window at
// equal durations; 1.6 % without the hoisting, profiles/r04al_band_persist_nolicm.log).  The one-workgroup forms keep
// the hoisting (this build of them is 1.4 % slower per iteration).
namespace {
// The single-demand-period instantiation's launch: launch_band_one_q's persistent grid (the resident slots measured for
// this kernel, DVH_BAND_RESERVE, the zeroed queue counter) over pdhg_band_kernel_j1, reported as the form's variant
// code + kBandJ1.  (A launcher of its own, so that the ICE unit, which shares launch_band_one_q, is built as before.)
template <bool GATE, bool BOX>
hipError_t launch_band_persist_j1(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                                  const int32_t* list, int nlist, int* variant_out) {
  constexpr int B = kBandSteps / 3, S = 3;
  const size_t lds = band_lds_bytes(B, S, false, true);
  auto kern = pdhg_band_kernel_j1<B, S, false, true, 2, GATE, BOX>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const int count = list ? nlist : ch.count;
  if (count <= 0) return hipSuccess;
  int& slots = w.slots[8 + (GATE ? 2 : 0) + (BOX ? 1 : 0)];
  if (slots <= 0) {
    int nb = 0, cus = 0, dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)kern, B, lds)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    slots = std::max(1, nb) * std::max(1, cus);
  }
  static const int reserve = [] { const char* e = getenv("DVH_BAND_RESERVE"); return e ? std::max(0, atoi(e)) : 0; }();
  const int grid = std::min(count, std::max(1, slots - 2 * reserve));
  if ((e = hipMemsetAsync(w.queue, 0, sizeof(int32_t), s)) != hipSuccess) return e;
  const BandArgs args{b, w, ch, o, list, count, w.queue};
  hipLaunchKernelGGL(kern, dim3(grid), dim3(B), lds, s, args);
  if (variant_out) *variant_out = 9000000 + 1000 * (S - 1) + kBandJ1 + B / kWave;
  return hipGetLastError();
}
}  // namespace
// j1: the list holds no battery window with J != 1 (counted by the host from the descriptors, dvh_solve.cpp
// scan_chunks): the single-demand-period instantiation takes it, unless DVH_BAND_J1=0 (read at every launch, A/B)
hipError_t launch_band_persist(bool gate, bool box, bool j1, const Batch& b, const Work& w, const Chunk& ch,
                               const Opts& o, hipStream_t s, const int32_t* list, int nlist, int* variant_out) {
  constexpr int B = kBandSteps / 3;
  if (j1) {
    const char* e = getenv("DVH_BAND_J1");
    if (e && atoi(e) == 0) j1 = false;
  }
  if (j1) {
    if (gate) {
      if (box) return launch_band_persist_j1<true, true>(b, w, ch, o, s, list, nlist, variant_out);
      return launch_band_persist_j1<true, false>(b, w, ch, o, s, list, nlist, variant_out);
    }
    if (box) return launch_band_persist_j1<false, true>(b, w, ch, o, s, list, nlist, variant_out);
    return launch_band_persist_j1<false, false>(b, w, ch, o, s, list, nlist, variant_out);
  }
  if (gate) {
    if (box) return launch_band_one_q<B, 3, false, true, 2, true, true, true>(b, w, ch, o, s, list, nlist, variant_out);
    return launch_band_one_q<B, 3, false, true, 2, true, false, true>(b, w, ch, o, s, list, nlist, variant_out);
  }
  if (box) return launch_band_one_q<B, 3, false, true, 2, false, true, true>(b, w, ch, o, s, list, nlist, variant_out);
  return launch_band_one_q<B, 3, false, true, 2, false, false, true>(b, w, ch, o, s, list, nlist, variant_out);
}
#elif DVH_BAND_PERSIST_TU == 2
hipError_t launch_band_persist_ice(bool gate, bool box, const Batch& b, const Work& w, const Chunk& ch, const Opts& o,
                                   hipStream_t s, const int32_t* list, int nlist, int* variant_out) {
  constexpr int B = kBandSteps;
  if (gate) {
    if (box) return launch_band_one_q<B, 1, true, false, 3, true, true, true>(b, w, ch, o, s, list, nlist, variant_out);
    return launch_band_one_q<B, 1, true, false, 3, true, false, true>(b, w, ch, o, s, list, nlist, variant_out);
  }
  if (box) return launch_band_one_q<B, 1, true, false, 3, false, true, true>(b, w, ch, o, s, list, nlist, variant_out);
  return launch_band_one_q<B, 1, true, false, 3, false, false, true>(b, w, ch, o, s, list, nlist, variant_out);
}
#else
hipError_t launch_pdhg_band(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s, bool ice,
                            int form, bool box, const int32_t* list, int nlist, bool j1, int* variant_out) {
  if (ice) {
    if (box) return launch_band_one<kBandSteps, 1, true, false, 3, true>(b, w, ch, o, s, list, nlist, false, variant_out);
    return launch_band_one<kBandSteps, 1, true, false, 3>(b, w, ch, o, s, list, nlist, false, variant_out);
  }
  if (form == 1) {  // (the one-step form has no single-demand-period instantiation)
    if (box) return launch_band_one<kBandSteps, 1, false, false, 3, true>(b, w, ch, o, s, list, nlist, false, variant_out);
    return launch_band_one<kBandSteps, 1, false, false, 3>(b, w, ch, o, s, list, nlist, false, variant_out);
  }
  if (box) return launch_band_one<kBandSteps / 3, 3, false, true, 2, true>(b, w, ch, o, s, list, nlist, j1, variant_out);
  return launch_band_one<kBandSteps / 3, 3, false, true, 2>(b, w, ch, o, s, list, nlist, j1, variant_out);
}
#endif

}  // namespace dvh
