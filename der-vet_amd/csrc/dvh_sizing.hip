// dvh_sizing.hip -- device-side builder of the reliability sizing LP (Reliability.size_for_outages,
// dervet/MicrogridValueStreams/Reliability.py:221-274; include/dervet_hip.h dvh_sizing_windows), written from the
// resident series straight into the packed batch in HBM.
//
// One 256-thread workgroup per LP, one thread per (window, step) at a time.  Every value is formed with the
// operations of dervet_hip/lp/sizing.py sizing_lp in its order, so the arrays are bit-identical to the host path
// (tests/test_gpu_sizing.py).  Layout, for K starts and L steps:
//   columns   [E, P | per window w: ch[0..L-1], dis[0..L-1], s[0..L-1]]
//   rows      K L equalities (4 entries each), then 5 per (w, k) >= rows (2 entries each): nnz = 14 K L.
#include <math.h>

// Bit-identity with numpy needs every product rounded before it is added: no FMA contraction in this file.
#pragma clang fp contract(off)
#include "dvh_internal.h"

namespace dvh {
namespace {

constexpr int kSizeB = 256;

__global__ __launch_bounds__(kSizeB) void build_sizing_kernel(const SizingLP* lps, const int64_t* desc,
                                                             int32_t* indptr, int32_t* indices, double* data,
                                                             double* c, double* c0, double* q, double* l, double* u) {
  const int b = blockIdx.x;
  const SizingLP p = lps[b];
  const int64_t* d = desc + 8 * (int64_t)b;
  const int tid = threadIdx.x;
  const int K = p.K, L = p.L, KL = K * L;
  if (p.new_start >= 0) {  // the start this round adds (uniform branch)
    if (tid == 0) p.starts[K - 1] = p.new_start;
    __syncthreads();
  }
  int32_t* ip = indptr + d[4];
  int32_t* ix = indices + d[5];
  double* dv = data + d[5];
  double* cv = c + d[6];
  double* lv = l + d[6];
  double* uv = u + d[6];
  double* qv = q + d[7];
  // ---- row pointers
  for (int r = tid; r <= 6 * KL; r += kSizeB) ip[r] = r <= KL ? 4 * r : 4 * KL + 2 * (r - KL);
  const double ech = -(p.rte * p.dt);
  for (int e = tid; e < KL; e += kSizeB) {
    const int w = e / L, k = e - w * L;
    const int base = 2 + 3 * w * L;
    const int ch = base + k, dis = base + L + k, s = base + 2 * L + k;
    // ---- equality row: s_k - s_{k-1} - rte dt ch_k + dt dis_k = 0 (s_{-1} = a0 E)
    int o = 4 * e;
    if (k == 0) {
      ix[o] = 0;
      ix[o + 1] = ch;
      ix[o + 2] = dis;
      dv[o] = -p.a0;
      dv[o + 1] = ech;
      dv[o + 2] = p.dt;
    } else {
      ix[o] = ch;
      ix[o + 1] = dis;
      ix[o + 2] = s - 1;
      dv[o] = ech;
      dv[o + 1] = p.dt;
      dv[o + 2] = -1.0;
    }
    ix[o + 3] = s;
    dv[o + 3] = 1.0;
    qv[e] = 0.0;
    // ---- >= rows: ulsoc E - s_k, s_k - llsoc E, P - ch_k, P - dis_k, dis_k - ch_k >= d
    o = 4 * KL + 10 * e;
    ix[o] = 0;
    dv[o] = p.ulsoc;
    ix[o + 1] = s;
    dv[o + 1] = -1.0;
    ix[o + 2] = 0;
    dv[o + 2] = -p.llsoc;
    ix[o + 3] = s;
    dv[o + 3] = 1.0;
    ix[o + 4] = 1;
    dv[o + 4] = 1.0;
    ix[o + 5] = ch;
    dv[o + 5] = -1.0;
    ix[o + 6] = 1;
    dv[o + 6] = 1.0;
    ix[o + 7] = dis;
    dv[o + 7] = -1.0;
    ix[o + 8] = ch;
    dv[o + 8] = -1.0;
    ix[o + 9] = dis;
    dv[o + 9] = 1.0;
    const int i = p.starts[w] + k;
    double dem = 0.0;
    if (i < p.n_steps) {
      double cl = p.cl[i];
      if (p.shed) cl = cl * (p.shed[k] / 100.0);
      dem = cl - p.dg_gen;
      dem = dem - (p.pv_vari ? p.pv_vari[i] : 0.0);
    }
    double* qi = qv + KL + 5 * e;
    qi[0] = 0.0;
    qi[1] = 0.0;
    qi[2] = 0.0;
    qi[3] = 0.0;
    qi[4] = dem;
    // ---- dispatch columns: free of cost, in [0, inf)
    cv[ch] = 0.0;
    cv[dis] = 0.0;
    cv[s] = 0.0;
    lv[ch] = 0.0;
    lv[dis] = 0.0;
    lv[s] = 0.0;
    uv[ch] = INFINITY;
    uv[dis] = INFINITY;
    uv[s] = INFINITY;
  }
  if (tid == 0) {
    cv[0] = p.cE;
    cv[1] = p.cP;
    lv[0] = p.lE;
    uv[0] = p.uE;
    lv[1] = p.lP;
    uv[1] = p.uP;
    c0[b] = p.c0;
  }
}

__global__ void gather_sizes_kernel(const int64_t* desc, const double* x, const int32_t* istats, int nlp,
                                    double* sizes) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nlp) return;
  const int64_t off = desc[8 * (int64_t)b + 6];
  sizes[4 * b] = x[off];
  sizes[4 * b + 1] = x[off + 1];
  sizes[4 * b + 2] = (double)istats[2 * b];
  sizes[4 * b + 3] = (double)istats[2 * b + 1];
}

}  // namespace

hipError_t launch_build_sizing(const SizingLP* d_lps, int nlp, const int64_t* desc, int32_t* indptr, int32_t* indices,
                               double* data, double* c, double* c0, double* q, double* l, double* u, hipStream_t s) {
  if (nlp <= 0) return hipSuccess;
  hipLaunchKernelGGL(build_sizing_kernel, dim3(nlp), dim3(kSizeB), 0, s, d_lps, desc, indptr, indices, data, c, c0, q,
                     l, u);
  return hipGetLastError();
}

hipError_t launch_gather_sizes(const int64_t* desc, const double* x, const int32_t* istats, int nlp, double* sizes,
                               hipStream_t s) {
  if (nlp <= 0) return hipSuccess;
  hipLaunchKernelGGL(gather_sizes_kernel, dim3((nlp + 255) / 256), dim3(256), 0, s, desc, x, istats, nlp, sizes);
  return hipGetLastError();
}

}  // namespace dvh
