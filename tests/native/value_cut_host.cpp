// Host build of the economic-sizing arithmetic (der-vet_amd/csrc/dvh_value_cut.h, the routines
// csrc/dvh_value_sizing.hip runs) and of the entry points' argument validation, for tests/test_value_sizing_native.py:
//   g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared -I der-vet_amd/csrc value_cut_host.cpp
#include <cstring>
#include <vector>

#include "dvh_value_cut.h"
#include "dvh_value_sizing_validate.h"

using namespace dvh;

extern "C" {

// The cuts of G windows of one battery group laid out one after the other (window g's vectors at g * n, g * m,
// g * nnz); E .. ulsoc [G]; emax [G * T] or null; out [G][kCutCols].
void vc_window_cuts(int T, int J, int mI, int G, const int32_t* dcm_t, const int32_t* dcm_j, const int32_t* ix,
                    const double* dv, const double* c, const double* l, const double* u, const double* q,
                    const double* x, const double* y, const double* c0, const double* E, const double* P,
                    const double* soc_target, const double* llsoc, const double* ulsoc, const double* emax,
                    double* out) {
  const int64_t n = 3 * (int64_t)T + J, m = (int64_t)T + 1 + mI, nnz = 4 * (int64_t)T + 3 * (int64_t)mI;
  std::vector<double> z((size_t)T);
  for (int g = 0; g < G; ++g) {
    vc::CutIn in;
    in.T = T;
    in.J = J;
    in.mI = mI;
    in.dcm_t = dcm_t;
    in.dcm_j = dcm_j;
    in.ix = ix + g * nnz;
    in.dv = dv + g * nnz;
    in.c = c + g * n;
    in.l = l + g * n;
    in.u = u + g * n;
    in.x = x + g * n;
    in.q = q + g * m;
    in.y = y + g * m;
    in.c0 = c0[g];
    in.E = E[g];
    in.P = P[g];
    in.soc_target = soc_target[g];
    in.llsoc = llsoc[g];
    in.ulsoc = ulsoc[g];
    in.emax = emax ? emax + (int64_t)g * T : nullptr;
    vc::window_cut(in, z.data(), out + (int64_t)g * vc::kCutCols);
  }
}

// out = {E, P, theta, objective}; returns master_solve's status
int vc_master(int n, const double* cut, double cE, double cP, double alpha, double Elo, double Ehi, double Plo,
              double Phi, double* out) {
  vc::MasterIn in;
  in.n = n;
  in.cut = cut;
  in.cE = cE;
  in.cP = cP;
  in.alpha = alpha;
  in.Elo = Elo;
  in.Ehi = Ehi;
  in.Plo = Plo;
  in.Phi = Phi;
  return vc::master_solve(in, out);
}

// the message of validate_value_spec ("" when valid) into buf
void vc_validate_spec(const dvh_value_spec* s, char* buf, int len) {
  const std::string msg = validate_value_spec(*s, 0);
  std::strncpy(buf, msg.c_str(), (size_t)len - 1);
  buf[len - 1] = 0;
}

}  // extern "C"
