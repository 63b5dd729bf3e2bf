// dvh_certify.hip -- infeasibility / unboundedness certificates for on-chip windows (gfx950), opt-in
// (dvh_options.certify, dvh_certify_batch); restated for tests in tests/certify_ref.py.
//
// The restarted PDHG kernels can prove a window optimal; an infeasible one (a load above the import limit plus the
// discharge rating, a stretch the stored energy cannot carry under a POI limit, a min-SOE the charger cannot reach)
// runs to max_iters and comes back ITER_LIMIT or NUMERICAL.  This pass decides such windows: plain PDHG on the UNSCALED
// LP from a cold start (x = proj_[l,u](0), y = 0) with the diagonal Pock-Chambolle steps
//     tau_j = 1 / sum_i |K_ij|,  sigma_i = 1 / sum_j |K_ij|      (1 for an empty column / row)
//     x+ = proj(x - tau (c - K'y)),   y+ = y + sigma (q - K (2 x+ - x)),   >= rows' y clamped at 0.
// On an infeasible LP z_k - z_0 and z_{k+1} - z_k both converge to the infimal displacement vector: its dual part is a
// Farkas certificate, its primal part an unbounded ray.  Every kCertCheck iterations four candidates are tested, in
// this order: y_k, y_k - y_{k-1} (Farkas), x_k - x_0, x_k - x_{k-1} (ray); the pass stops at the first that passes, or
// at the cap.
//   Farkas test of v: >= rows clamped at 0, scaled to ||v||_inf = 1, r = K'v;
//     viol = max r_j^+ over u_j = +inf, r_j^- over l_j = -inf;  margin = q'v - sum_j (r_j > 0 ? u_j r_j : l_j r_j) over
//     the finite bounds;  certified when margin > 0, viol <= 1e-8 margin (PDLP's ray tolerance) and
//     margin >= 1e-9 (sum |q_i v_i| + sum |bound r_j|) (round-off cannot certify a feasible window).
//   Ray test of d: d_j >= 0 where l_j is finite, <= 0 where u_j is finite, scaled to ||d||_inf = 1;
//     viol = max(||K_E d||_inf, ||(K_I d)^-||_inf);  certified when -c'd > 0, viol <= 1e-8 (-c'd), -c'd >= 1e-9 sum |c_j d_j|.
//
// ONE WORKGROUP PER WINDOW, 256 threads, FP64.  x, y and one scratch vector (2 x+ - x, then the scaled candidate a
// test gathers) live in LDS, sized from the batch's largest on-chip window so that small windows share a CU; K'y never
// leaves the registers of the column's owner.  K' comes from a deterministic CSR transpose into the pass's own
// workspace (counts, scan, stable fill by one wave in row-major order, as setup_kernel's); the last-step candidates go
// through that workspace too.  No floating-point atomics; every reduction runs in a fixed order (a lane's columns in
// order, wave butterflies, the waves in order), so rays, margins and iteration counts are bit-reproducible.
#include "dvh_device.h"

#include <math.h>

namespace dvh {

namespace {

constexpr int kCertB = 256;
constexpr int kCertNW = kCertB / kWave;
constexpr int kCertCheck = 64;     // iterations between certificate tests
constexpr int kCertU = 4;          // rows a lane works on side by side (cert_rows)
constexpr double kRayTol = 1e-8;   // viol <= kRayTol * margin
constexpr double kFloor = 1e-9;    // margin >= kFloor * (sum of the absolute terms it is the difference of)
constexpr int kUndecided = 5;      // DVH_UNDECIDED

// Rows of a CSR matrix (K by rows, or K' by columns): rows of up to kLongRow entries one per thread, longer ones (the
// demand charge's tau column) one per wave with a shuffle tree.  f(p) -> the entry's term; g(row, sum) consumes it (by
// one lane).  Fixed order: a short row's entries in order; a long row's by lane stride, then the butterfly.
template <class F, class G>
__device__ __forceinline__ void cert_rows(const int32_t* ptr, int rows, const int* longl, int nlong, F f, G g) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // (kCertU rows of a lane side by side, entry q of each in turn: kCertU independent load chains in flight, every
  // row still summed in its own order)
  for (int i0 = tid; i0 < rows; i0 += kCertU * kCertB) {
    int s[kCertU], len[kCertU], mx = 0;
    double acc[kCertU];
#pragma unroll
    for (int u = 0; u < kCertU; ++u) {
      const int i = i0 + u * kCertB;
      s[u] = 0;
      len[u] = -1;  // (-1: no row, or a long one)
      acc[u] = 0.0;
      if (i < rows) {
        s[u] = ptr[i];
        const int l = ptr[i + 1] - s[u];
        if (l <= kLongRow) len[u] = l;
      }
      mx = max(mx, len[u]);
    }
    for (int q = 0; q < mx; ++q) {
#pragma unroll
      for (int u = 0; u < kCertU; ++u)
        if (q < len[u]) acc[u] += f(s[u] + q);
    }
#pragma unroll
    for (int u = 0; u < kCertU; ++u)
      if (len[u] >= 0) g(i0 + u * kCertB, acc[u]);
  }
  for (int L = wid; L < nlong; L += kCertNW) {
    const int i = longl[L];
    const int s = ptr[i], e = ptr[i + 1];
    double acc = 0.0;
    for (int p = s + lane; p < e; p += kWave) acc += f(p);
    acc = wave_sum(acc);
    if (lane == 0) g(i, acc);
  }
}

// max over the workgroup (identical in every thread); red holds kCertNW doubles
__device__ __forceinline__ double cert_block_max(double v, double* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < kCertNW; ++w) r = fmax(r, red[w]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ bool cert_passes(double margin, double viol, double scale) {
  return margin > 0.0 && viol <= kRayTol * margin && margin >= kFloor * scale;
}

__global__ __launch_bounds__(kCertB) void certify_kernel(const Batch b, const CertWork cw, const int count,
                                                         const int cap, const int gate, const int small_max) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double red[(kCertNW + 1) * 4];
  __shared__ int sh_wt[kCertNW];
  __shared__ int longr[kLMax], longc[kLMax];
  __shared__ int sh_cnt[2];
  const int k = blockIdx.x;
  if (k >= count) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // after a solve (gate): only what the cascade left undecided
  if (gate) {
    const int st = b.istats[2 * k];
    if (st != kIterLimit && st != kNumerical) return;
  }
  const int64_t* d = b.desc + 8 * (int64_t)k;
  const int n = (int)d[0], m = (int)d[1], meq = (int)d[2], nnz = (int)d[3];
  const int64_t on = d[6], om = d[7];
  auto finish = [&](int status, int iters, double s0, double margin, double viol) {
    if (tid != 0) return;
    b.istats[2 * k] = status;
    if (!gate) b.istats[2 * k + 1] = iters;  // (after a solve the main solve's count stays)
    b.stats[4 * k] = s0;
    b.stats[4 * k + 1] = margin;
    b.stats[4 * k + 2] = viol;
    b.stats[4 * k + 3] = 0.0;
  };
  auto undecided = [&](int iters) {  // the screen reports it; after a solve the window stays exactly as it was
    if (!gate) finish(kUndecided, iters, NAN, 0.0, 0.0);
  };
  if (n > small_max || m > small_max) {  // medium tier and grid-wide windows: skipped, counted
    if (tid == 0) atomicAdd(&cw.counts[3], 1);
    undecided(0);
    return;
  }
  if (tid == 0) atomicAdd(&cw.counts[0], 1);

  const int32_t* Kp = b.indptr + d[4];
  const int32_t* Kc = b.indices + d[5];
  const double* Kv = b.data + d[5];
  const double* cc = b.c + on;
  const double* lo = b.l + on;
  const double* up = b.u + on;
  const double* qq = b.q + om;
  int32_t* Tp = cw.tptr + (on - cw.base_n) + k;
  int32_t* Ti = cw.tind + (d[5] - cw.base_nz);
  double* Tv = cw.tval + (d[5] - cw.base_nz);
  double* tau = cw.tau + (on - cw.base_n);
  double* gx = cw.gx + (on - cw.base_n);
  double* sig = cw.sig + (om - cw.base_m);
  double* gy = cw.gy + (om - cw.base_m);
  double* xs = reinterpret_cast<double*>(smem);  // [n]
  double* ys = xs + n;                           // [m]
  double* ss = ys + m;                           // [max(n, m)]; first the transpose cursors, n + 1 ints
  int32_t* cursor = reinterpret_cast<int32_t*>(ss);

  // 0. crossed bounds (the setup step reports them before a solve; the screen meets them here): no iteration needed
  {
    double cr = 0.0;
    for (int j = tid; j < n; j += kCertB) cr = fmax(cr, lo[j] - up[j]);
    cr = cert_block_max(cr, red);
    if (cr > 0.0) {
      if (tid == 0) atomicAdd(&cw.counts[1], 1);
      finish(1, 0, INFINITY, cr, 0.0);
      return;
    }
  }
  // 1. K' (CSC of K): column counts (integer, order-independent), exclusive scan, stable fill
  for (int j = tid; j <= n; j += kCertB) cursor[j] = 0;
  __syncthreads();
  for (int p = tid; p < nnz; p += kCertB) {
    const int j = Kc[p];
    if ((unsigned)j < (unsigned)n) atomicAdd(&cursor[j], 1);
  }
  __syncthreads();
  {
    const int per = (n + kCertB - 1) / kCertB;
    const int s0 = min(n, tid * per), e0 = min(n, s0 + per);
    int acc = 0;
    for (int j = s0; j < e0; ++j) acc += cursor[j];
    int inc = acc;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int t = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += t;
    }
    if (lane == kWave - 1) sh_wt[wid] = inc;
    __syncthreads();
    int run = inc - acc;
    for (int u = 0; u < wid; ++u) run += sh_wt[u];
    for (int j = s0; j < e0; ++j) {
      const int v = cursor[j];
      Tp[j] = run;
      cursor[j] = run;
      run += v;
    }
    if (tid == kCertB - 1) Tp[n] = run;
  }
  __syncthreads();
  // wave 0 walks the entries in row-major order, 64 at a time; entries of one column inside a chunk are ranked by lane
  // (one ballot per bit of the column index), so every column's entries land in row order
  if (wid == 0) {
    const int nb = 32 - __builtin_clz((unsigned)(n > kWave ? n : kWave));
    for (int base = 0; base < nnz; base += kWave) {
      const int p = base + lane;
      bool v = p < nnz;
      int j = v ? Kc[p] : -1 - lane;
      if (v && (unsigned)j >= (unsigned)n) {  // (a column index outside the window: dropped, as in the counts)
        v = false;
        j = -1 - lane;
      }
      unsigned long long eq = ~0ull;
      for (int bt = 0; bt < nb; ++bt) {
        const bool bit = (j >> bt) & 1;
        const unsigned long long bal = __ballot(bit);
        eq &= bit ? bal : ~bal;
      }
      {
        const bool neg = j < 0;
        const unsigned long long bal = __ballot(neg);
        eq &= neg ? bal : ~bal;
      }
      const int rank = __popcll(eq & ((1ull << lane) - 1ull)), cnt = __popcll(eq);
      int pos = 0, row = 0;
      if (v) {
        pos = cursor[j] + rank;
        int a = 0, e = m;  // the entry's row: the last i with Kp[i] <= p
        while (e - a > 1) {
          const int mid = (a + e) >> 1;
          if (Kp[mid] <= p) a = mid; else e = mid;
        }
        row = a;
      }
      __builtin_amdgcn_wave_barrier();
      if (v) {
        Ti[pos] = row;
        Tv[pos] = Kv[p];
        if (rank == cnt - 1) cursor[j] = pos + 1;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  // 2. long rows / columns (deterministic ballot compaction by wave 0)
  if (wid == 0) {
    int nr = 0, nc = 0;
    for (int base = 0; base < m; base += kWave) {
      const int i = base + lane;
      const bool isl = i < m && (Kp[i + 1] - Kp[i]) > kLongRow;
      const unsigned long long bal = __ballot(isl);
      const int pre = __popcll(bal & ((1ull << lane) - 1ull));
      if (isl && nr + pre < kLMax) longr[nr + pre] = i;
      nr += __popcll(bal);
    }
    for (int base = 0; base < n; base += kWave) {
      const int j = base + lane;
      const bool isl = j < n && (Tp[j + 1] - Tp[j]) > kLongRow;
      const unsigned long long bal = __ballot(isl);
      const int pre = __popcll(bal & ((1ull << lane) - 1ull));
      if (isl && nc + pre < kLMax) longc[nc + pre] = j;
      nc += __popcll(bal);
    }
    if (lane == 0) {
      sh_cnt[0] = nr;
      sh_cnt[1] = nc;
    }
  }
  __syncthreads();
  const int nlr = sh_cnt[0], nlc = sh_cnt[1];
  if (nlr > kLMax || nlc > kLMax) {  // more dense rows than the lists hold (setup_kernel's limit too): not decided
    undecided(0);
    return;
  }
  // 3. steps and the cold start
  cert_rows(Tp, n, longc, nlc, [&](int p) { return fabs(Tv[p]); },
            [&](int j, double a) {
              tau[j] = a > 0.0 ? 1.0 / a : 1.0;
              xs[j] = fmin(fmax(0.0, lo[j]), up[j]);
            });
  cert_rows(Kp, m, longr, nlr, [&](int p) { return fabs(Kv[p]); },
            [&](int i, double a) {
              sig[i] = a > 0.0 ? 1.0 / a : 1.0;
              ys[i] = 0.0;
            });
  __syncthreads();

  // Farkas test of the candidate in src (ys, or the last step in gy); the scaled candidate stays in ss
  auto farkas = [&](const double* src, double& margin, double& viol) -> bool {
    double nv = 0.0;
    for (int i = tid; i < m; i += kCertB) {
      double v = src[i];
      if (i >= meq) v = fmax(v, 0.0);
      nv = fmax(nv, fabs(v));
    }
    const double nrm = cert_block_max(nv, red);
    if (!(nrm > 0.0) || !(nrm < INFINITY)) return false;  // (false for NaN too)
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // q'v, sum |q_i v_i|, sum bound r_j, sum |bound r_j|
    double vl = 0.0;
    for (int i = tid; i < m; i += kCertB) {
      double v = src[i];
      if (i >= meq) v = fmax(v, 0.0);
      v = v / nrm;
      ss[i] = v;
      const double t = qq[i] * v;
      acc[0] += t;
      acc[1] += fabs(t);
    }
    __syncthreads();
    cert_rows(Tp, n, longc, nlc, [&](int p) { return Tv[p] * ss[Ti[p]]; },
              [&](int j, double r) {
                if (r > 0.0) {
                  const double u = up[j];
                  if (u < INFINITY) {
                    acc[2] += u * r;
                    acc[3] += fabs(u * r);
                  } else {
                    vl = fmax(vl, r);
                  }
                } else if (r < 0.0) {
                  const double l = lo[j];
                  if (l > -INFINITY) {
                    acc[2] += l * r;
                    acc[3] += fabs(l * r);
                  } else {
                    vl = fmax(vl, -r);
                  }
                }
              });
    block_sum<kCertB, 4>(acc, red);
    viol = cert_block_max(vl, red);
    margin = acc[0] - acc[2];
    return cert_passes(margin, viol, acc[1] + acc[3]);
  };
  // Ray test of x - x_0 (last = false) or of the last step in gx
  auto ray = [&](bool last, double& descent, double& viol) -> bool {
    auto cand = [&](int j) {
      const double l = lo[j], u = up[j];
      double v = last ? gx[j] : xs[j] - fmin(fmax(0.0, l), u);
      if (l > -INFINITY) v = fmax(v, 0.0);
      if (u < INFINITY) v = fmin(v, 0.0);
      return v;
    };
    double nv = 0.0;
    for (int j = tid; j < n; j += kCertB) nv = fmax(nv, fabs(cand(j)));
    const double nrm = cert_block_max(nv, red);
    if (!(nrm > 0.0) || !(nrm < INFINITY)) return false;
    double acc[2] = {0.0, 0.0};  // c'd, sum |c_j d_j|
    double vl = 0.0;
    for (int j = tid; j < n; j += kCertB) {
      const double v = cand(j) / nrm;
      ss[j] = v;
      const double t = cc[j] * v;
      acc[0] += t;
      acc[1] += fabs(t);
    }
    __syncthreads();
    cert_rows(Kp, m, longr, nlr, [&](int p) { return Kv[p] * ss[Kc[p]]; },
              [&](int i, double a) { vl = fmax(vl, i < meq ? fabs(a) : -a); });
    block_sum<kCertB, 2>(acc, red);
    viol = cert_block_max(vl, red);
    descent = -acc[0];
    return cert_passes(descent, viol, acc[1]);
  };

  // 4. the iteration
  int it = 0;
  while (it < cap) {
    ++it;
    const bool check = (it % kCertCheck) == 0;
    cert_rows(Tp, n, longc, nlc, [&](int p) { return Tv[p] * ys[Ti[p]]; },
              [&](int j, double r) {
                const double xo = xs[j];
                const double xn = fmin(fmax(xo - tau[j] * (cc[j] - r), lo[j]), up[j]);
                xs[j] = xn;
                ss[j] = 2.0 * xn - xo;
                if (check) gx[j] = xn - xo;
              });
    __syncthreads();
    cert_rows(Kp, m, longr, nlr, [&](int p) { return Kv[p] * ss[Kc[p]]; },
              [&](int i, double a) {
                const double yo = ys[i];
                double yn = yo + sig[i] * (qq[i] - a);
                if (i >= meq) yn = fmax(yn, 0.0);
                ys[i] = yn;
                if (check) gy[i] = yn - yo;
              });
    __syncthreads();
    if (!check) continue;
    double margin = 0.0, viol = 0.0;
    if (m > 0 && (farkas(ys, margin, viol) || farkas(gy, margin, viol))) {
      if (b.y)
        for (int i = tid; i < m; i += kCertB) b.y[om + i] = ss[i];
      if (tid == 0) {
        atomicAdd(&cw.counts[1], 1);
        atomicMax(&cw.counts[4], it);
      }
      finish(1, it, INFINITY, margin, viol);
      return;
    }
    if (ray(false, margin, viol) || ray(true, margin, viol)) {
      for (int j = tid; j < n; j += kCertB) b.x[on + j] = ss[j];
      if (tid == 0) {
        atomicAdd(&cw.counts[2], 1);
        atomicMax(&cw.counts[4], it);
      }
      finish(2, it, -INFINITY, margin, viol);
      return;
    }
    __syncthreads();  // ss is the next iteration's again
  }
  undecided(it);
}

}  // namespace

size_t certify_lds_bytes(int max_n, int max_m) {
  return align16(sizeof(double) * ((size_t)max_n + (size_t)max_m + (size_t)(max_n > max_m ? max_n : max_m) + 1));
}

hipError_t launch_certify(const Batch& b, const CertWork& cw, int count, int max_n, int max_m, int cap, int gate,
                          hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const size_t lds = certify_lds_bytes(max_n, max_m);
  hipError_t e = hipFuncSetAttribute((const void*)certify_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(certify_kernel, dim3(count), dim3(kCertB), lds, s, b, cw, count, cap, gate, kSmallMax);
  return hipGetLastError();
}

}  // namespace dvh
