// Economic sizing arithmetic, shared by the device kernels (csrc/dvh_value_sizing.hip) and the host build the tests
// compile (tests/native/value_cut_host.cpp): the optimality cut of one solved battery window in the sizes (E, P), and the
// exact solve of a case's three-variable master LP over its cuts (include/dervet_hip.h, "Economic sizing").
//
// The cut.  For a window solved at s = (E, P) with duals y (>= rows clamped at 0), r = c - K'y, weak duality gives
//   V(s') >= D(s') = q(s')'y + sum_j [ l_j(s') r_j^+ - u_j(s') r_j^- ] + c0          for every s',
// a term whose bound is infinite dropped and the largest |r_j| that points at one reported as rinf.  Of the battery
// window (dervet_hip/lp/builder.py battery_group; dvh_build.hip) only q_0 = q_T = soc_target E, u_ch = u_dis = P,
// l_ene = llsoc E and u_ene = min(ulsoc E, emax_t) depend on s, so D is convex in s' and its linearisation at s is a cut:
//   g_E = soc_target (y_0 + y_T) + sum_t [ llsoc r_ene,t^+ - ulsoc r_ene,t^- (ulsoc E <= emax_t) ]
//   g_P = -sum_t (r_ch,t^- + r_dis,t^-),      a = D(s) - g_E E - g_P P.
// K'y is formed from the battery pattern's known column structure -- ch_t / dis_t / ene_t meet the SOE rows t and t + 1
// and the demand-charge rows of step t, tau_j the rows of period j -- with the CSR indices checked against it
// (check_rows); the demand-charge rows must come period by period with ascending steps (the builder's order), which
// check_rows verifies too, so that a step meets at most one row per period and z_t = sum of its rows' duals is formed
// by one add per period, in period order.
//
// Every floating-point operation is one IEEE operation in the order written here (no contraction: the pragma below and
// -ffp-contract=off), and the sums are formed the way a 256-thread workgroup forms them -- lane l adds the terms of
// t = l, l + 256, .. in order, each wave halves its 64 partials (l += l + 32, + 16, ..), the four wave sums are added in
// wave order -- which window_cut() walks serially, so host and device agree bit for bit.
//
// The master.  min cE E + cP P + alpha theta  s.t.  theta >= a_k + gE_k E + gP_k P (k < n), E and P in their boxes,
// alpha > 0, solved by a dual simplex over the n + 4 constraints with a three-constraint basis (3 x 3 solves by
// Cramer's rule): start at the box corner that one cut alone makes optimal, then bring in the most violated constraint
// (lowest index on ties; the lowest violated index once the iteration count passes n + 4, Bland's rule) until none is
// violated.  Serial and deterministic; at most kMaxCuts cuts.
#pragma once
#include <math.h>

#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#ifndef DVH_HD
#if defined(__HIPCC__)
#define DVH_HD __host__ __device__
#else
#define DVH_HD
#endif
#endif

namespace dvh {
namespace vc {

constexpr int kCutLanes = 256;  // threads of a cut workgroup
constexpr int kWaveLanes = 64;
constexpr int kCutCols = 10;    // DVH_VALUE_CUT_COLS
constexpr int kMaxCuts = 256;   // DVH_VALUE_MAX_CUTS
constexpr int kMaxJ = 64;       // DVH_VALUE_MAX_J
// columns of a window's cut
enum { cA = 0, cGE, cGP, cDobj, cPobj, cRinf, cFlag, cStatus, cIters, cReserved };
// lane sums of a cut
enum { sQy = 0, sBound, sGE, sCh, sDis, sCx, kCutSums };
// window flags (cFlag, summed): the window is not read, its cut is NaN
constexpr int kBadShape = 1;    // descriptor is not the group's battery shape, or the window lies outside the arrays
constexpr int kBadPattern = 2;  // a CSR row is not the battery pattern's, or the demand-charge rows are out of order
constexpr int kBadRating = 4;   // pch != pdis

DVH_HD inline double qnan() { return __builtin_nan(""); }
DVH_HD inline double max2(double a, double b) { return b > a ? b : a; }
DVH_HD inline bool finite(double v) { return v - v == 0.0; }

// One solved window, every pointer at the window's own first entry.
struct CutIn {
  int T, J, mI;
  const int32_t* dcm_t;  // [mI]
  const int32_t* dcm_j;  // [mI]
  const int32_t* ix;     // [4T + 3mI] CSR column indices
  const double* dv;      // [4T + 3mI] CSR values
  const double* c;       // [3T + J]
  const double* l;
  const double* u;
  const double* q;       // [T + 1 + mI]
  const double* x;
  const double* y;
  double c0;
  double E, P, soc_target, llsoc, ulsoc;
  const double* emax;    // [T] or null
  DVH_HD int fin() const { return 1 + 4 * (T - 1); }  // first entry of the end-of-window row
  DVH_HD int dcm0() const { return fin() + 3; }        // first entry of the demand-charge rows
};

// the dual of row i as the cut uses it: a >= row's clamped at 0 (the result contract returns them so)
DVH_HD inline double row_dual(const CutIn& in, int i) {
  const double v = in.y[i];
  return (i > in.T && v < 0.0) ? 0.0 : v;
}

// The pattern check of lane `lane`: its SOE rows and demand-charge rows.  0 when they are the battery pattern's.
DVH_HD inline int check_rows(const CutIn& in, int lane, int lanes) {
  const int T = in.T;
  int bad = 0;
  if (lane == 0) {
    const int f = in.fin();
    if (in.ix[0] != 2 * T || in.ix[f] != T - 1 || in.ix[f + 1] != 2 * T - 1 || in.ix[f + 2] != 3 * T - 1) bad = kBadPattern;
  }
  for (int t = lane; t < T - 1; t += lanes) {
    const int p = 1 + 4 * t;
    if (in.ix[p] != t || in.ix[p + 1] != T + t || in.ix[p + 2] != 2 * T + t || in.ix[p + 3] != 2 * T + t + 1)
      bad = kBadPattern;
  }
  const int d0 = in.dcm0();
  for (int i = lane; i < in.mI; i += lanes) {
    const int t = in.dcm_t[i], j = in.dcm_j[i], p = d0 + 3 * i;
    if (t < 0 || t >= T || j < 0 || j >= in.J) {
      bad = kBadPattern;
      continue;
    }
    if (in.ix[p] != t || in.ix[p + 1] != T + t || in.ix[p + 2] != 3 * T + j) bad = kBadPattern;
    if (in.dv[p] != -1.0 || in.dv[p + 1] != 1.0 || in.dv[p + 2] != 1.0) bad = kBadPattern;
    if (i > 0) {  // period by period, ascending steps
      const int tp = in.dcm_t[i - 1], jp = in.dcm_j[i - 1];
      if (jp > j || (jp == j && tp >= t)) bad = kBadPattern;
    }
  }
  return bad;
}

// Pass j of the demand-charge rows by lane `lane`: z[t] += the dual of the period's row at step t (at most one per
// step, so the lanes never meet); returns the lane's part of the period's dual sum (tau_j's K'y).
DVH_HD inline double scatter_pass(const CutIn& in, int j, int lane, int lanes, double* z) {
  double acc = 0.0;
  for (int i = lane; i < in.mI; i += lanes)
    if (in.dcm_j[i] == j) {
      const double yi = row_dual(in, in.T + 1 + i);
      z[in.dcm_t[i]] += yi;
      acc += yi;
    }
  return acc;
}

// l r^+ - u r^- of one column, an infinite bound dropped into rinf
DVH_HD inline double bound_term(double r, double l, double u, double* rinf) {
  if (r > 0.0) {
    if (finite(l)) return l * r;
    *rinf = max2(*rinf, r);
  } else if (r < 0.0) {
    if (finite(u)) return u * r;
    *rinf = max2(*rinf, -r);
  }
  return 0.0;
}

// r of ch_t, dis_t, ene_t (z: the demand-charge duals of the steps)
DVH_HD inline void step_reduced(const CutIn& in, const double* z, int t, double* rch, double* rdis, double* rene) {
  const int T = in.T;
  const bool last = t == T - 1;
  const int p = last ? in.fin() : 1 + 4 * t;
  const double yr = row_dual(in, t + 1);
  const double kch = in.dv[p] * yr + (-z[t]);
  const double kdis = in.dv[p + 1] * yr + z[t];
  const double up = t == 0 ? in.dv[0] * row_dual(in, 0) : in.dv[1 + 4 * (t - 1) + 3] * row_dual(in, t);
  const double kene = up + in.dv[p + 2] * yr;
  *rch = in.c[t] - kch;
  *rdis = in.c[T + t] - kdis;
  *rene = in.c[2 * T + t] - kene;
}

// The sums of lane `lane` over its rows and steps; rinf: its largest |r| at an infinite bound.
DVH_HD inline void lane_sums(const CutIn& in, const double* z, int lane, int lanes, double* s, double* rinf) {
  const int T = in.T, m = T + 1 + in.mI;
  for (int u = 0; u < kCutSums; ++u) s[u] = 0.0;
  *rinf = 0.0;
  for (int i = lane; i < m; i += lanes) s[sQy] += in.q[i] * row_dual(in, i);
  for (int t = lane; t < T; t += lanes) {
    double rch, rdis, rene;
    step_reduced(in, z, t, &rch, &rdis, &rene);
    s[sBound] += bound_term(rch, in.l[t], in.u[t], rinf);
    s[sBound] += bound_term(rdis, in.l[T + t], in.u[T + t], rinf);
    s[sBound] += bound_term(rene, in.l[2 * T + t], in.u[2 * T + t], rinf);
    if (rene > 0.0) s[sGE] += in.llsoc * rene;
    if (rene < 0.0 && (!in.emax || in.ulsoc * in.E <= in.emax[t])) s[sGE] += in.ulsoc * rene;
    if (rch < 0.0) s[sCh] += -rch;
    if (rdis < 0.0) s[sDis] += -rdis;
    s[sCx] += in.c[t] * in.x[t];
    s[sCx] += in.c[T + t] * in.x[T + t];
    s[sCx] += in.c[2 * T + t] * in.x[2 * T + t];
  }
}

// The cut from the workgroup's totals; tausum[j]: the dual sum of period j's rows.
DVH_HD inline void finish_cut(const CutIn& in, const double* tot, double rinf, const double* tausum, double* out) {
  const int T = in.T;
  double cx = tot[sCx], bound = tot[sBound];
  for (int j = 0; j < in.J; ++j) {
    const double r = in.c[3 * T + j] - tausum[j];
    bound += bound_term(r, in.l[3 * T + j], in.u[3 * T + j], &rinf);
    cx += in.c[3 * T + j] * in.x[3 * T + j];
  }
  const double dobj = (tot[sQy] + bound) + in.c0;
  const double gE = in.soc_target * (row_dual(in, 0) + row_dual(in, T)) + tot[sGE];
  const double gP = -(tot[sCh] + tot[sDis]);
  out[cA] = (dobj - gE * in.E) - gP * in.P;
  out[cGE] = gE;
  out[cGP] = gP;
  out[cDobj] = dobj;
  out[cPobj] = cx + in.c0;
  out[cRinf] = rinf;
}

DVH_HD inline void bad_cut(int flag, double* out) {
  for (int u = 0; u < kCutCols; ++u) out[u] = qnan();
  out[cFlag] = (double)flag;
  out[cStatus] = out[cIters] = out[cReserved] = 0.0;
}

// What the workgroup's reduction leaves in lane 0: each wave halves its partials, the waves are added in order.
inline double tree_sum(const double* part) {
  double tot = 0.0;
  for (int w = 0; w < kCutLanes / kWaveLanes; ++w) {
    double v[kWaveLanes];
    for (int i = 0; i < kWaveLanes; ++i) v[i] = part[w * kWaveLanes + i];
    for (int o = kWaveLanes / 2; o > 0; o >>= 1)
      for (int i = 0; i < o; ++i) v[i] += v[i + o];
    tot = w == 0 ? v[0] : tot + v[0];
  }
  return tot;
}

// One window's cut on the host, in the kernel's order.  z: [T] scratch.  out [kCutCols]; cFlag != 0: a bad window.
inline void window_cut(const CutIn& in, double* z, double* out) {
  int bad = in.J > kMaxJ ? kBadShape : 0;
  for (int lane = 0; lane < kCutLanes && !bad; ++lane) bad |= check_rows(in, lane, kCutLanes);
  if (bad) {
    bad_cut(bad, out);
    return;
  }
  double part[kCutSums][kCutLanes], tausum[kMaxJ], tot[kCutSums];
  for (int t = 0; t < in.T; ++t) z[t] = 0.0;
  for (int j = 0; j < in.J; ++j) {
    for (int lane = 0; lane < kCutLanes; ++lane) part[0][lane] = scatter_pass(in, j, lane, kCutLanes, z);
    tausum[j] = tree_sum(part[0]);
  }
  double rinf = 0.0;
  for (int lane = 0; lane < kCutLanes; ++lane) {
    double s[kCutSums], ri;
    lane_sums(in, z, lane, kCutLanes, s, &ri);
    for (int u = 0; u < kCutSums; ++u) part[u][lane] = s[u];
    rinf = max2(rinf, ri);
  }
  for (int u = 0; u < kCutSums; ++u) tot[u] = tree_sum(part[u]);
  finish_cut(in, tot, rinf, tausum, out);
  out[cFlag] = out[cStatus] = out[cIters] = out[cReserved] = 0.0;
}

// ---- the master LP

struct MasterIn {
  int n;             // cuts, 1 .. kMaxCuts
  const double* cut; // [n][3] = {a, gE, gP}
  double cE, cP, alpha;
  double Elo, Ehi, Plo, Phi;
};
// master_solve's status
constexpr int kMasterOk = 0, kMasterIterLimit = 1, kMasterSingular = 2;

// constraint k of the master as normal . z >= rhs, z = (E, P, theta): k < n the cuts, then E >= Elo, -E >= -Ehi,
// P >= Plo, -P >= -Phi
DVH_HD inline void master_row(const MasterIn& in, int k, double* nrm, double* rhs) {
  const int n = in.n;
  if (k < n) {
    nrm[0] = -in.cut[3 * k + 1];
    nrm[1] = -in.cut[3 * k + 2];
    nrm[2] = 1.0;
    *rhs = in.cut[3 * k];
    return;
  }
  nrm[0] = nrm[1] = nrm[2] = 0.0;
  if (k == n) { nrm[0] = 1.0; *rhs = in.Elo; }
  else if (k == n + 1) { nrm[0] = -1.0; *rhs = -in.Ehi; }
  else if (k == n + 2) { nrm[1] = 1.0; *rhs = in.Plo; }
  else { nrm[1] = -1.0; *rhs = -in.Phi; }
}

DVH_HD inline double det3(const double* a, const double* b, const double* c) {
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// out = {E, P, theta, objective cE E + cP P + alpha theta}
DVH_HD inline int master_solve(const MasterIn& in, double* out) {
  const int n = in.n, nc = n + 4;
  const double cost[3] = {in.cE, in.cP, in.alpha};
  // with cut 0 alone the optimum is the corner the signs of cE + alpha gE, cP + alpha gP point away from
  int B[3];
  B[0] = 0;
  B[1] = (in.cE + in.alpha * in.cut[1] >= 0.0) ? n : n + 1;
  B[2] = (in.cP + in.alpha * in.cut[2] >= 0.0) ? n + 2 : n + 3;
  const int cap = 8 * nc + 64;
  for (int it = 0; it < cap; ++it) {
    double N[3][3], b[3];
    for (int u = 0; u < 3; ++u) master_row(in, B[u], N[u], &b[u]);
    // the vertex: N z = b (rows); by Cramer over the columns
    double col[3][3];
    for (int u = 0; u < 3; ++u)
      for (int v = 0; v < 3; ++v) col[v][u] = N[u][v];
    const double det = det3(col[0], col[1], col[2]);
    if (!(det != 0.0) || !finite(det)) return kMasterSingular;
    double z[3];
    z[0] = det3(b, col[1], col[2]) / det;
    z[1] = det3(col[0], b, col[2]) / det;
    z[2] = det3(col[0], col[1], b) / det;
    // a box side in the basis holds exactly
    for (int u = 0; u < 3; ++u) {
      if (B[u] == n) z[0] = in.Elo;
      if (B[u] == n + 1) z[0] = in.Ehi;
      if (B[u] == n + 2) z[1] = in.Plo;
      if (B[u] == n + 3) z[1] = in.Phi;
    }
    // the most violated constraint (Bland's lowest index once the count says the walk may be cycling)
    const bool bland = it > nc;
    int enter = -1;
    double worst = 0.0;
    for (int k = 0; k < nc; ++k) {
      if (k == B[0] || k == B[1] || k == B[2]) continue;
      double nr[3], rhs;
      master_row(in, k, nr, &rhs);
      const double lhs = (nr[0] * z[0] + nr[1] * z[1]) + nr[2] * z[2];
      const double scale = 1.0 + fabs(rhs) + fabs(nr[0] * z[0]) + fabs(nr[1] * z[1]) + fabs(z[2]);
      const double viol = (rhs - lhs) / scale;
      if (viol > 1e-13 && (enter < 0 || (!bland && viol > worst))) {
        enter = k;
        worst = viol;
        if (bland) break;
      }
    }
    if (enter < 0) {
      out[0] = z[0];
      out[1] = z[1];
      out[2] = z[2];
      out[3] = (in.cE * z[0] + in.cP * z[1]) + in.alpha * z[2];
      return kMasterOk;
    }
    // multipliers of the basis: cost = sum mu_u N_u; the entering normal = sum w_u N_u  (N' mu = cost: the rows as columns)
    double ne[3], rhs;
    master_row(in, enter, ne, &rhs);
    double mu[3], w[3];
    mu[0] = det3(cost, N[1], N[2]) / det3(N[0], N[1], N[2]);
    mu[1] = det3(N[0], cost, N[2]) / det3(N[0], N[1], N[2]);
    mu[2] = det3(N[0], N[1], cost) / det3(N[0], N[1], N[2]);
    w[0] = det3(ne, N[1], N[2]) / det3(N[0], N[1], N[2]);
    w[1] = det3(N[0], ne, N[2]) / det3(N[0], N[1], N[2]);
    w[2] = det3(N[0], N[1], ne) / det3(N[0], N[1], N[2]);
    int leave = -1;
    double best = 0.0;
    for (int u = 0; u < 3; ++u) {
      if (!(w[u] > 1e-14)) continue;
      const double ratio = max2(mu[u], 0.0) / w[u];
      if (leave < 0 || ratio < best || (ratio == best && B[u] < B[leave])) {
        leave = u;
        best = ratio;
      }
    }
    if (leave < 0) return kMasterSingular;  // the entering constraint cannot be met: crossed box
    B[leave] = enter;
  }
  return kMasterIterLimit;
}

}  // namespace vc
}  // namespace dvh
