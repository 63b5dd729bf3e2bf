/*
 * dervet_hip.h -- C ABI of libdervet_hip, the MI355X batched dispatch-LP solver.
 *
 * Drop-in boundary.  In the reference every optimization window is solved by
 *   storagevet Scenario.solve_optimization(functions, constraints) -> (cvx_problem, obj_expressions, cvx_error_msg)
 * called once per window from the serial loop at dervet/MicrogridScenario.py:310-320 (optimize_problem_loop,
 * :281), i.e. CVXPY 1.0.31 canonicalisation + ECOS 2.0.7 / GLPK (cvxopt 1.2.5) in C (requirements.txt:1,2,5).
 * This library replaces that solve for LP windows: the caller exports every window's canonical LP
 *     min c'x + c0   s.t.  K_E x = q_E,  K_I x >= q_I,  l <= x <= u      (rows ordered E then I)
 * and solves all windows of all scenarios as ONE batch with a restarted reflected-Halpern PDHG
 * (PDLP family) in hand-written HIP for gfx950.  No pointers are retained after a call returns.
 *
 * Entry point  <->  reference interface it replaces
 *   dvh_create / dvh_destroy   : solver construction (cvx.Problem(...).solve(solver=...) picks ECOS/GLPK;
 *                                storagevet Scenario.solve_optimization, called at MicrogridScenario.py:319)
 *   dvh_solve_batch            : the per-window prob.solve() of MicrogridScenario.py:319, for `count`
 *                                windows at once (host buffers in / out)
 *   dvh_solve_packed_device    : same, on a batch already resident in HBM (bench / torch callers)
 *   dvh_last_error             : cvx_error_msg (errors travel as a message, MicrogridScenario.py:319-320)
 *   result.status              : maps to the cvxpy status strings read by save_optimization_results
 *                                (MicrogridScenario.py:348-363): OPTIMAL->"optimal",
 *                                PRIMAL_INFEASIBLE->"infeasible", DUAL_INFEASIBLE->"unbounded",
 *                                ITER_LIMIT->"optimal_inaccurate", NUMERICAL->"solver_error".
 *
 * Threading: one handle per host thread.  A handle drives every GPU whose bit is set in device_mask (0 = device 0):
 * dvh_solve_batch splits a host-buffer batch into contiguous ranges of near-equal estimated cost, one per device,
 * solved concurrently by one host thread per device (no inter-device traffic; each device writes its windows'
 * results straight into the caller's dvh_result buffers).  Device-resident batches (dvh_solve_packed_device) and
 * the reliability sweep run on the handle's first device.  Multi-process runs (one rank per GPU, torch.distributed
 * / RCCL all-gather of the results) use one single-device handle per rank.
 * Return codes: 0 = OK, negative = usage / HIP error (message via dvh_last_error).
 */
#ifndef DERVET_HIP_H
#define DERVET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVH_OK 0
#define DVH_ERR_ARG (-1)
#define DVH_ERR_HIP (-2)
#define DVH_ERR_UNSUPPORTED (-3)

/* per-window status */
#define DVH_OPTIMAL 0
#define DVH_PRIMAL_INFEASIBLE 1
#define DVH_DUAL_INFEASIBLE 2
#define DVH_ITER_LIMIT 3
#define DVH_NUMERICAL 4
#define DVH_UNDECIDED 5 /* dvh_certify_batch only: neither certificate found within the cap */

/* structure hints (dvh_lp.structure) */
#define DVH_STRUCT_GENERIC_CSR 0
#define DVH_STRUCT_BATTERY_BANDED 1

typedef struct dvh_options {
  double eps;                 /* relative KKT tolerance (primal, dual, gap), default 1e-6          */
  int32_t max_iters;          /* per window, default 100000                                       */
  int32_t check_every;        /* restart-check period (iterations), default 32                    */
  int32_t ruiz_iters;         /* Ruiz equilibration passes, default 10                            */
  int32_t power_iters;        /* power-iteration steps for ||K||_2, default 64                    */
  double step_safety;         /* eta = step_safety / ||K||_2, default 0.998                       */
  double reflection;          /* Halpern reflection rho in [0,1], default 1                       */
  double restart_sufficient;  /* default 0.2  */
  double restart_necessary;   /* default 0.8  */
  double restart_artificial;  /* default 0.1  */
  double primal_weight_theta; /* default 1.0  */
  int32_t verbose;            /* 0 silent                                                           */
  int32_t kkt_every;          /* termination (KKT) check every kkt_every restart checks, default 4 */
  int32_t warm_start;         /* 1: start each window from the x / y already in the output buffers     */
                              /*    (unscaled, e.g. a similar window's solution); 0: x = proj(0), y = 0 */
  int32_t certify_iters;      /* iteration cap of the certificate pass (certify below); 0 = default, 65536          */
  double eps_obj;             /* objective-error termination (0 = off), default 1e-6: besides the KKT test, */
                              /* |pobj - dobj| + ||y||_2 ||r_p||_2 + sum_j |r_d,j| |x_j| <= eps_obj (1 + |pobj|) */
                              /* (unscaled), an estimate of |pobj - opt|: the gap, the dual-weighted primal   */
                              /* residual, and what the dual residual r_d = c - K'y - lambda lets the dual    */
                              /* objective overstate the optimum by.  The band kernel's ICE form (config-5    */
                              /* windows) applies the test without the last term                              */
  int32_t kkt_predict;        /* 0 = off (default).  P > 0 (band and ELL kernels; the other tiers ignore it): a  */
                              /* due KKT check is skipped while its predicted outcome, the last check's worst   */
                              /* ratio max(pres, dres, gap) / eps scaled by the fixed-point residual's decrease  */
                              /* since then, exceeds P; at most 4 due checks in a row are skipped.  Termination  */
                              /* still needs a KKT check that passes: this only saves hopeless checks.           */
  int32_t certify;            /* 0 = off (default: nothing new is launched or allocated).  1: after the last tier  */
                              /* of a solve, the certificate pass (dvh_certify_batch below) runs over the batch's  */
                              /* on-chip windows that came back ITER_LIMIT or NUMERICAL, in one launch gated on    */
                              /* the device (no extra host wait): a window it certifies returns PRIMAL_INFEASIBLE  */
                              /* or DUAL_INFEASIBLE with its ray, every other window is left exactly as it was     */
                              /* 2: everything 1 means, plus an early exit inside the PDHG kernels that take       */
                              /* POI windows (the generic kernel; the band kernel's interconnection form): at every */
                              /* KKT check the dual of T(z_k) is put through the Farkas test below, and a window    */
                              /* that passes stops there as PRIMAL_INFEASIBLE with iters = that check's iteration,  */
                              /* its ray in y, stats as the pass writes them and an x that means nothing.  The      */
                              /* pass still follows and skips such a window by its status.  The battery band, ICE,  */
                              /* ELL, chain and grid-wide tiers ignore the level (their windows keep the pass), as  */
                              /* do unbounded windows.  Feasible windows return what levels 0 and 1 return.         */
} dvh_options;

typedef struct dvh_lp {
  int32_t n;                  /* variables                          */
  int32_t m_eq;               /* equality rows (first)              */
  int32_t m_ineq;             /* >= rows (after the equalities); m_eq + m_ineq >= 1 (a window without a row is   */
                              /* rejected with a message); rows and columns without an entry are allowed        */
  int32_t nnz;
  const int32_t* indptr;      /* [m_eq + m_ineq + 1] CSR row pointers (0-based)                  */
  const int32_t* indices;     /* [nnz] column indices                                           */
  const double* data;         /* [nnz]                                                          */
  const double* c;            /* [n] objective                                                  */
  double c0;                  /* objective constant                                             */
  const double* q;            /* [m] right-hand side                                            */
  const double* l;            /* [n] lower bounds (-INFINITY allowed)                           */
  const double* u;            /* [n] upper bounds (+INFINITY allowed)                           */
  int32_t structure;          /* DVH_STRUCT_* hint (informational)                              */
  int32_t reserved;
} dvh_lp;

/* x, y: the candidate T(z_k) of the window's last termination check, unscaled; obj and the three relative KKT numbers
 * are that check's, computed from the same x, y (lambda: the part of c - K'y the finite bounds carry: all of it on a
 * boxed column, its positive part with a lower bound only, its negative part with an upper bound only, none on a free
 * column; pobj = c'x + c0; dobj = q'y + sum_j l_j max(lambda_j, 0) + sum_j u_j min(lambda_j, 0) + c0; >= rows count
 * max(q - Kx, 0)).  DVH_OPTIMAL: the three numbers are <= eps and the eps_obj test holds (dvh_options).
 * DVH_ITER_LIMIT: a termination check always runs at the limit -- the check period is min(check_every, max_iters) on
 * every tier and in both host restatements (oracle/) -- so x, y and the numbers are those of a checked candidate at or
 * before max_iters, never unset.  x is clipped to [l, u] on the way out (the unscaling can round past a bound).
 * The numbers are NaN only where no iteration ran: a window reported DVH_NUMERICAL by the set-up (more than 64 rows or
 * columns of more than 32 entries), with x, y untouched; a crossed-bounds window (PRIMAL_INFEASIBLE, 0 iterations)
 * has obj NaN and the others 0.  A window that ends DVH_NUMERICAL while iterating (a non-finite objective) returns the
 * diverged candidate: its x, y may hold NaN or infinities and mean nothing.  tests/kkt_ref.py recomputes all of it on
 * the host (tests/test_gpu_result_contract.py, tests/test_gpu_planted.py). */
typedef struct dvh_result {
  double* x;                  /* caller-allocated [n] or NULL                                   */
  double* y;                  /* caller-allocated [m] or NULL (duals; >= rows have y >= 0)       */
  double obj;                 /* c'x + c0                                                       */
  double primal_res_rel;      /* ||(q - Kx)_proj||_2 / (1 + ||q||_2)                            */
  double dual_res_rel;        /* ||c - K'y - lambda||_2 / (1 + ||c||_2)                         */
  double gap_rel;             /* |pobj - dobj| / (1 + |pobj| + |dobj|)                          */
  int32_t status;             /* DVH_OPTIMAL ...                                                */
  int32_t iters;
} dvh_result;

/* A batch already resident in device memory ("packed" layout).
 * desc[8*k + 0..7] = {n, m, m_eq, nnz, off_row, off_nz, off_n, off_m} (int64) for window k:
 *   indptr[off_row .. off_row+m]   (window-local row pointers, int32)
 *   indices/data[off_nz .. +nnz]   (window-local column indices int32 / values f64)
 *   c,l,u[off_n .. +n], q[off_m .. +m], c0[k]
 * Outputs: x[off_n..], y[off_m..], stats[4k..4k+3] = {obj, primal_res_rel, dual_res_rel, gap_rel},
 *          istats[2k..2k+1] = {status, iters}.  All pointers are device pointers. */
typedef struct dvh_packed {
  int32_t count;
  int32_t reserved;
  int64_t total_n, total_m, total_nnz, total_rows; /* sizes of the concatenated arrays (rows = sum(m+1)) */
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
} dvh_packed;

typedef struct dvh_handle dvh_handle;

const char* dvh_version(void);
void dvh_default_options(dvh_options* opts);
int dvh_create(int device_mask, const dvh_options* opts, dvh_handle** out);
/* The same with an explicit device list (devices may repeat: several concurrent sub-handles on one GPU). */
int dvh_create_devices(const int32_t* devices, int32_t n, const dvh_options* opts, dvh_handle** out);
/* Devices (sub-handles) of a handle. */
int dvh_device_count(const dvh_handle* h);
int dvh_destroy(dvh_handle* h);
const char* dvh_last_error(const dvh_handle* h);
int dvh_set_options(dvh_handle* h, const dvh_options* opts);

/* ---- The result all-gather across ranks.  One process per GPU: the windows are sharded over the
 * ranks with no traffic during the solve, then ONE all-gather returns every window's result row (objective,
 * residuals, status, iterations, (scenario, window) tag, dispatch) to every rank.  Replaces the reference's serial
 * case loop (dervet/DERVET.py:75-83).  RCCL is opened at run time (librccl.so.1 of /opt/rocm, or DVH_RCCL_LIB);
 * DVH_ERR_UNSUPPORTED when it cannot be.
 *   dvh_comm_unique_id: rank 0 draws the 128-byte id (ncclGetUniqueId) the launcher hands to every rank;
 *   dvh_comm_init: joins rank `rank` of `world` on the handle's device (single-device handles only);
 *   dvh_comm_info: {rank, world} (0, 0 without a communicator);
 *   dvh_gather_results: out[world * bytes_per_rank] (device) = every rank's rows[bytes_per_rank] (device) in rank
 *     order; asynchronous on `stream` (a hipStream_t; NULL = the handle's solver stream, i.e. after its solves). */
#define DVH_COMM_ID_BYTES 128
int dvh_comm_unique_id(dvh_handle* h, uint8_t* id);
int dvh_comm_init(dvh_handle* h, int32_t rank, int32_t world, const uint8_t* id);
int dvh_comm_info(const dvh_handle* h, int32_t* rank_world);
int dvh_gather_results(dvh_handle* h, const void* rows, uint64_t bytes_per_rank, void* out, void* stream);

/* Host buffers in / out.  Blocks until the batch is solved. */
int dvh_solve_batch(dvh_handle* h, const dvh_lp* lps, int32_t count, dvh_result* out);

/* Device-resident batch; `stream` is a hipStream_t (NULL = the handle's own stream).  Asynchronous
 * w.r.t. the host when stream != NULL; call dvh_synchronize / hipStreamSynchronize before reading. */
int dvh_solve_packed_device(dvh_handle* h, const dvh_packed* batch, void* stream);

/* ---- Device-side window builder (the LP that storagevet's
 * set_up_optimization builds for a battery + demand-charge + retail / DA window, MicrogridScenario.py:322-346).
 * Expands G windows' inputs (device pointers) into the packed batch's LP arrays, windows first .. first + G - 1,
 * whose descriptors the caller has set (n = 3T + J, m = T + 1 + mI, nnz = 4T + 3 mI, any offsets; ICE below).  The values are
 * exactly those of dervet_hip/lp/builder.py battery_group (same formulas, same summation order; bit-identical,
 * tests/test_gpu_builder.py), so a sweep ships its compact inputs to HBM instead of the expanded LPs.
 * Asynchronous on the handle's stream. */
typedef struct dvh_battery_group {
  int32_t T, J, G, mI;             /* steps, demand-charge (tau) columns, windows, demand-charge rows           */
  double dt;                       /* hours per step                                                             */
  int32_t has_retail, has_da;      /* price inputs present                                                       */
  int32_t has_emin, has_emax;      /* aggregate-SOE limits present                                               */
  const int32_t* dcm_t;            /* [mI] step of each demand-charge row (rows in builder order)                */
  const int32_t* dcm_j;            /* [mI] its tau column                                                        */
  const double* base;              /* [G*T] net load + housekeeping power, kW (load - fixed PV + hp)             */
  const double* retail;            /* [G*T] $/kWh or NULL                                                        */
  const double* da;                /* [G*T] $/kWh or NULL                                                        */
  const double* demand;            /* [G*J] $/kW                                                                 */
  const double* emin;              /* [G*T] kWh or NULL                                                          */
  const double* emax;              /* [G*T] kWh or NULL                                                          */
  const double* E;                 /* [G] energy capacity, kWh                                                   */
  const double* pch;               /* [G] kW                                                                     */
  const double* pdis;              /* [G] kW                                                                     */
  const double* rte;               /* [G] round-trip efficiency, fraction                                        */
  const double* sdr;               /* [G] self-discharge, fraction per hour (sdr % / 100)                        */
  const double* soc_target;        /* [G] fraction                                                               */
  const double* ulsoc;             /* [G] fraction                                                               */
  const double* llsoc;             /* [G] fraction                                                               */
  const double* om;                /* [G] variable O&M, $/MWh                                                    */
  const double* c0;                /* [G] objective constant (the terms' constants, summed on the host)          */
  /* LP-relaxed ICE (BASELINE config 5; builder.battery_group `ice`): columns elec_t, on_t after tau (n = 5T + J),
   * elec_t in every demand-charge row (4 entries), two >= rows per step after them (m = 3T + 1 + mI,
   * nnz = 8T + 4 mI): cap on_t - elec_t >= 0, elec_t - pmin on_t >= 0; elec in [0, inf), on in [0, 1].  */
  int32_t has_ice, pad_ice;
  const double* ice_cap;           /* [G] rated power x units, kW                                                */
  const double* ice_pmin;          /* [G] minimum stable power x units, kW                                       */
  const double* ice_cost;          /* [G] (efficiency x fuel cost + variable O&M) x dt, $/kW per step             */
  /* One electric vehicle (builder.battery_group `ev`; not with has_ice): columns ev_ch_t, ev_ene_t after tau
   * (n = 5T + J), -ev_ch_t in every demand-charge row (4 entries), and after the battery's T + 1 equality rows, step by
   * step, an optional one-entry start row and the step's load row (m_eq = 2T + 1 + D with D start rows, m = m_eq + mI).
   * ev_code is a HOST array: per step the sum of DVH_EV_* flags.  The library validates it against the descriptors
   * (DVH_ERR_ARG, nothing launched) and scans it into the rows' offsets.  The reference's own rows and the cycle
   * layout: dervet_hip/lp/builder.py _add_ev.  dvh_value_cuts refuses has_ev (DVH_ERR_UNSUPPORTED).                  */
  int32_t has_ev, pad_ev;
  const double* ev_ch_max;         /* [G] kW                                                                     */
  const double* ev_target;         /* [G] kWh per session                                                        */
  const int32_t* ev_code;          /* host [T]                                                                   */
} dvh_battery_group;
#define DVH_EV_PLUGGED 1           /* ev_ch_t <= ev_ch_max (else ev_ch_t = 0)                                    */
#define DVH_EV_START 2             /* a start row ev_ene_t = 0 precedes the step's load row ...                  */
#define DVH_EV_START_TARGET 4      /* ... its right-hand side is ev_target instead                               */
#define DVH_EV_LAST 8              /* the last step of a cycle: the load row has no ev_ene_{t+1}, rhs 0 ...      */
#define DVH_EV_END_TARGET 16       /* ... or ev_target ...                                                       */
#define DVH_EV_END_R 32            /* ... or R = (steps with DVH_EV_TRAIL) dt ev_ch_max                          */
#define DVH_EV_TRAIL 64            /* a step of the session cut by the window's end: ev_ene_t <= R               */
int dvh_build_battery_group(dvh_handle* h, const dvh_battery_group* group, const dvh_packed* batch, int32_t first);
int dvh_synchronize(dvh_handle* h);

/* ---- Synthetic scenario series on the device (BASELINE.json configs 4 / 5; no reference
 * counterpart: the reference reads one time-series CSV per case, dervet/DERVET.py:75-83, and a sweep's perturbed
 * series are this framework's workload generator, dervet_hip/lp/scenarios.py).  Draws, per scenario, exactly what
 * numpy's np.random.Generator(np.random.PCG64(seed)) draws on the host: one standard normal (the lognormal load
 * scale), `steps` standard normals filtered as scipy.signal.lfilter([1], [1, a1]) with the innovations after the
 * first scaled by `innov`, then `n_uniform` next_double words (uniform(low, high) = low + (high - low) * u).
 * seeds: host [count] SeedSequence entropy; z0 [count], ar [count * steps], uniform [count * n_uniform]: device.
 * Bit-identical to the host generator (tests/test_gpu_series.py).  DVH_ERR_UNSUPPORTED if a wedge test of the
 * ziggurat fell within 2^-40 of the device exp (its outcome could differ from the host libm's; not observed).
 * Returns after the kernel completed. */
typedef struct dvh_sweep_draws {
  int32_t count, steps, n_uniform;
  const uint64_t* seeds;
  double a1;                       /* lfilter denominator coefficient a[1] (-phi)                              */
  double innov;                    /* innovation scale of steps >= 1 (sqrt(1 - phi^2))                         */
  double* z0;
  double* ar;
  double* uniform;
  /* optional [count] int32 (device): 1 for a scenario whose ziggurat wedge test landed within 2^-40 of exp() (its
   * draws may differ from numpy's), else 0.  Given, such scenarios are only flagged (the caller regenerates them on
   * the host) and the call returns DVH_OK; NULL: any such scenario fails the call with DVH_ERR_UNSUPPORTED. */
  int32_t* ambiguous;
} dvh_sweep_draws;
int dvh_series_draws(dvh_handle* h, const dvh_sweep_draws* d);

/* The device builder's inputs (dvh_battery_group base / retail / c0) of G windows cut from the scenarios' series:
 * window k of scenario rows[k] covers steps t0 .. t0 + T - 1 (rep steps per hour of the hourly series);
 *   base[k][t]   = (site_load[h] * load_scale[s]) * (1 + 0.05 * ar[s][h]) - pv_rated[s] * pv_profile[h] + hp[s],
 *   retail[k][t] = price[t0 + t] * price_scale[s],                                  h = (t0 + t) / rep,
 *   c0[k]        = the retail term's constant sum((retail * dt) * base) as numpy sums it (in step order; pairwise
 *                  when G = 1), + c0_add[s]
 * (J > 0: the window has demand-charge columns, which add zero constants).  All pointers device; rows are
 * range-checked on the device (DVH_ERR_ARG).  Asynchronous on the handle's stream; returns after it completed. */
typedef struct dvh_window_series {
  int32_t G, T, t0, rep, J, count, hours;
  double dt;
  const int32_t* rows;             /* [G] scenario of each window, 0 <= rows[k] < count                        */
  const double* ar;                /* [count * hours] (dvh_series_draws)                                       */
  const double* site_load;         /* [hours] kW                                                                */
  const double* pv_profile;        /* [hours] kW per rated kW (NaN as 0)                                        */
  const double* price;             /* [>= t0 + T] energy price per step, $/kWh                                  */
  const double* load_scale;        /* [count]                                                                   */
  const double* price_scale;       /* [count]                                                                   */
  const double* pv_rated;          /* [count] kW                                                                */
  const double* hp;                /* [count] housekeeping power, kW                                            */
  const double* c0_add;            /* [count] fixed O&M x discharge rating                                      */
  double* base;                    /* out [G * T]                                                               */
  double* retail;                  /* out [G * T]                                                               */
  double* c0;                      /* out [G]                                                                   */
} dvh_window_series;
int dvh_series_windows(dvh_handle* h, const dvh_window_series* w);

/* ---- Seeded scenario sweeps (dervet_hip/sweep.py; the sensitivity cases of dervet/DERVET.py:75 solve the same
 * windows for many perturbed scenarios; no reference counterpart: the reference solves every window cold).
 * Warm starts for `count` windows of a device-resident packed batch from solved partner windows of the same LP
 * shape, in one launch on the handle's stream (ordered with the solves; returns after it completed).
 * pairs (host, int32 [count][3]): {window, partner window, T}.  x <- the partner's x scaled per column by
 * u_window / u_partner where both are finite and u_partner > 0, else copied; T > 0 (battery + DCM shape,
 * n = 3T + 1): the duals of rows 0..T scaled by mean|c_window[0:T]| / mean|c_partner[0:T]| and the others by
 * c_window[3T] / c_partner[3T] (denominators clamped at 1e-12); T <= 0: duals copied.  DVH_ERR_ARG for a pair
 * naming no window, a window listed twice, a partner that is itself listed (checked before the launch), or windows
 * of different shape (those pairs are skipped, the others applied). */
int dvh_warm_transfer(dvh_handle* h, const dvh_packed* batch, const int32_t* pairs, int32_t count);
/* The same from a weighted blend of q partners (1 <= q <= 8): rows[count][q + 2] = {window, partner_1 .. partner_q, T},
 * weights[count][q] (host; normally summing to 1): x = sum_k w_k x_k', y = sum_k w_k y_k' with x_k', y_k' partner k's
 * solution transferred as dvh_warm_transfer does (summed in row order).  q = 1 with weight 1 is dvh_warm_transfer bit
 * for bit.  DVH_ERR_ARG as dvh_warm_transfer, and for q out of range or a weight that is not finite. */
int dvh_warm_transfer_blend(dvh_handle* h, const dvh_packed* batch, const int32_t* rows, const double* weights,
                            int32_t count, int32_t q);

/* ---- Infeasibility / unboundedness certificates (no reference counterpart: ECOS / GLPK report "infeasible" or
 * "unbounded" themselves, cvxpy statuses read at MicrogridScenario.py:348-363; the restarted PDHG kernels can only
 * prove a window optimal, or infeasible when a column's bounds are crossed).  The pass runs plain PDHG on the
 * unscaled LP of every on-chip window (n, m <= 4096; one workgroup each), cold (x = proj(0), y = 0), with the
 * diagonal steps tau_j = 1 / sum_i |K_ij|, sigma_i = 1 / sum_j |K_ij|, and every 64 iterations tests y_k and
 * y_k - y_{k-1} as Farkas certificates and x_k - x_0 and x_k - x_{k-1} as unbounded rays (on an infeasible LP all
 * converge to the infimal displacement vector), until one passes or certify_iters iterations are done.
 *   Farkas (PRIMAL_INFEASIBLE): y with its >= rows clamped at 0 and ||y||_inf = 1, r = K'y,
 *     viol = max r_j^+ over u_j = +inf, r_j^- over l_j = -inf, margin = q'y - sum_j (r_j > 0 ? u_j r_j : l_j r_j) over
 *     the finite bounds; certified when margin > 0, viol <= 1e-8 margin, margin >= 1e-9 (sum |q_i y_i| + sum |bound r_j|).
 *   Ray (DUAL_INFEASIBLE): d with d_j >= 0 where l_j is finite, <= 0 where u_j is finite, ||d||_inf = 1,
 *     viol = max(||K_E d||_inf, ||(K_I d)^-||_inf); certified when -c'd > 0, viol <= 1e-8 (-c'd), -c'd >= 1e-9 sum |c_j d_j|.
 * A certified window: status 1 / 2, obj = +INFINITY / -INFINITY, primal_res_rel = margin (-c'd), dual_res_rel = viol,
 * gap_rel = 0 (stats = {+-INF, margin, viol, 0}), the normalised ray in y (status 1) or x (status 2), the other vector
 * untouched.  Bit-reproducible run to run (no floating-point atomics, fixed-order reductions).
 * dvh_certify_batch runs the pass alone over every listed window -- a screen to call before a solve: status 1 / 2 as
 * above with iters = the pass's iterations, else DVH_UNDECIDED (x, y untouched; windows above the on-chip size too).
 * A window whose bounds are crossed is PRIMAL_INFEASIBLE at 0 iterations with margin = the largest l_j - u_j and no
 * ray.  With dvh_options.certify = 1 the same pass follows every solve (dvh_solve_batch and dvh_solve_packed_device,
 * every kernel path, every device of the handle) over the windows left ITER_LIMIT / NUMERICAL; there iters stays the
 * main solve's.  Host buffers in / out; blocks; runs on the handle's first device. */
int dvh_certify_batch(dvh_handle* h, const dvh_lp* lps, int32_t count, dvh_result* out);
/* The certificate pass of the most recent solve / dvh_certify_batch: out5 = {windows examined (on-chip windows the pass
 * iterated on), certified primal infeasible, certified dual infeasible, skipped for size (n or m > 4096), largest
 * iteration count at which a certificate passed}.  All 0 when the pass did not run; reset by every solve. */
int dvh_last_certify(const dvh_handle* h, int32_t* out5);
/* Its kernel time (HIP events, milliseconds; 0 when it did not run). */
int dvh_last_certify_ms(const dvh_handle* h, double* ms);
/* dvh_options.certify = 2: out2 = {windows of the most recent solve certified inside a PDHG kernel, the largest
 * iteration count among them}.  They are not among dvh_last_certify's counts: the pass never examined them.  Both 0
 * below level 2; reset by every solve. */
int dvh_last_certify_early(const dvh_handle* h, int32_t* out2);

/* Timing of the most recent solve on the handle's stream (HIP events, milliseconds):
 * [0] whole solve, [1] setup kernel (transpose + scaling + power iteration), [2] PDHG kernels.  On the default
 * cascade the band kernels scale the windows they take themselves, inside the PDHG launch, and the setup kernel runs
 * only for what they refuse, between the cascade's PDHG launches: there [1] is ~0 and [2] holds all of it (setup
 * included); the A/B paths (dvh_set_kernel_path 1 / 2) run setup_kernel first and split the two as written. */
int dvh_last_timing(const dvh_handle* h, double* ms3);

/* Host waits on the stream during the most recent solve (dvh_solve_batch / dvh_solve_packed_device): the
 * descriptors' read-back (device batches), one per kernel tier that ran (the cascade's lists are formed on the
 * device, dvh_route.hip), the medium tier's hand-offs, and the final wait for the results and timing events. */
int dvh_last_host_syncs(const dvh_handle* h, int32_t* out);
/* Kernel-path diagnostics of the most recent solve: out4 = {windows solved by the ELL fast kernel,
 * windows solved by the generic CSR kernel, kernel variant code, generic_only flag}. */
int dvh_last_stats(const dvh_handle* h, int32_t* out4);
/* Windows per solver path in the most recent solve: out3 = {ELL kernel, generic CSR kernel, grid-wide
 * large-LP path (n or m > 4096: one window at a time over the whole GPU, e.g. BASELINE config 3)}. */
int dvh_last_path_counts(const dvh_handle* h, int32_t* out3);
/* The same plus the battery-banded kernel: out4 = {ELL kernel, generic CSR kernel, grid-wide large-LP path,
 * battery-banded kernel (windows with the storagevet battery + DCM structure, detected on the device)}. */
int dvh_last_path_counts4(const dvh_handle* h, int32_t* out4);
/* The same plus the medium tier: out5 = {ELL, generic, grid-wide, battery-banded, medium tier (battery windows of
 * 769 .. 12,288 steps -- the annual hourly window n = "year", sub-hourly monthly windows -- solved as a batch, a
 * team of one workgroup per <= 768-step segment per window, dvh_chain.hip)}. */
int dvh_last_path_counts5(const dvh_handle* h, int32_t* out5);
/* The instantiation of the battery-banded kernel that the most recent solve's battery pass ran: the kernel variant code
 * of dvh_last_stats, + 50 where the three-step form ran with the demand-period count fixed at 1 (no window of the
 * chunk had another; DVH_BAND_J1=0 in the environment keeps the run-time count); -1 where the pass took no window. */
int dvh_last_band_variant(const dvh_handle* h, int32_t* out);
/* Medium-tier team launches of the most recent solve that aborted (a segment exchange outlasted the spin limit): the
 * windows such a launch had finished keep their results, the others were solved on the grid-wide path, and the solve
 * still returns DVH_OK.  out = that count (0 when nothing aborted); reset by every solve. */
int dvh_last_chain_aborts(const dvh_handle* h, int32_t* out);
/* Diagnostics of a successful solve that took a fallback (a medium-tier abort: the workgroups' exchange state), or
 * "" -- dvh_last_error is left to errors.  Reset by every solve. */
const char* dvh_last_warning(const dvh_handle* h);
/* ---- Post-facto reliability sweep.
 * Replaces Reliability.load_coverage_probability (dervet/MicrogridValueStreams/Reliability.py:876-967) and the
 * serial recursion it drives (data_process :447-487, simulate_outage :489-570): for every case, an outage is
 * simulated from EVERY start step (one GPU thread each) and the covered lengths give the load coverage
 * probability curve P(outage of L hours covered), L = dt, 2 dt, .., max_outage.  The DER aggregates are the
 * caller's (Reliability.get_der_mix_properties :276-332): pv_vari = sum of pv_max x nu, gamma = largest gamma,
 * dg_gen = total ICE power (minus the largest unit for N-2), ESS limits = llsoc / ulsoc x energy rating. */
typedef struct dvh_outage_case {
  int32_t n_steps;                /* len(critical load)                                              */
  int32_t max_outage;             /* max_outage_duration (hours; also the data window in steps, :462) */
  double dt;                      /* hours per step                                                  */
  const double* critical_load;    /* [n_steps] kW                                                    */
  const double* pv_max;           /* [n_steps] total PV maximum generation, or NULL (no PV)          */
  const double* pv_vari;          /* [n_steps] total PV generation x nu, or NULL (no PV)             */
  const double* init_soe;         /* [n_steps] ESS energy at each outage start, or NULL: soe0        */
  const double* load_shed_pct;    /* [max_outage] % of the critical load kept per outage hour, or NULL */
  double soe0;                    /* energy at every start when init_soe == NULL (soc_init x rating) */
  double dg_gen;                  /* total generator power, kW (constant)                            */
  double gamma;                   /* largest PV gamma (fraction)                                     */
  double soe_min, soe_max;        /* ESS operation energy limits, kWh                                */
  double charge_max, discharge_max; /* kW                                                            */
  double rte;                     /* round-trip efficiency (fraction)                                */
} dvh_outage_case;

/* lengths: caller-allocated [sum n_steps] covered steps per start (case-major), or NULL;
 * lcp: caller-allocated [sum int(max_outage / dt)] load coverage probability per outage length.
 * Bit-exact with the reference's numpy arithmetic.  Blocks until done. */
int dvh_outage_coverage(dvh_handle* h, const dvh_outage_case* cases, int32_t count, int32_t* lengths,
                        double* lcp);
/* Reliability minimum-SOE requirement (Reliability.min_soe_iterative, Reliability.py:685-756, which feeds the
 * 'energy' 'min' system requirement of every window, :334-354): for every start step, an outage of
 * target_hours[k] (the Reliability 'target') simulated from soe0 (= soc_init x energy rating; init_soe and
 * load_shed_pct as above, init_soe ignored); min_soe[start] = max - min of its SOE profile including the start.
 * min_soe: caller-allocated [sum n_steps] (case-major).  Bit-exact with the numpy reference. */
int dvh_outage_min_soe(dvh_handle* h, const dvh_outage_case* cases, int32_t count, const int32_t* target_hours,
                       double* min_soe);
/* Kernel time of the last dvh_outage_coverage / dvh_outage_min_soe call (HIP events, milliseconds). */
int dvh_last_outage_ms(const dvh_handle* h, double* ms);

/* ---- Reliability sizing (Reliability.sizing_module, dervet/MicrogridValueStreams/Reliability.py:153-219): the
 * cutting-plane loop that sizes the ESS for an outage target -- solve a sizing LP over a set of outage starts
 * (size_for_outages :221-274), simulate an outage from every start of the series (find_first_uncovered :391-445), add
 * the first start the candidate size fails, repeat.
 *
 * The scan.  For every case, an outage of target_steps[k] steps simulated from every start from soe0 (init_soe
 * ignored, as in dvh_outage_min_soe; the per-step arithmetic of dvh_outage_coverage, bit-exact); a start t is
 * uncovered when covered < target_steps[k] and covered < n_steps - t (:431-435).  first[k] = the smallest uncovered
 * start or -1, n_uncovered[k] = their number (host arrays [count]; integer atomics, exact).  1 <= target_steps[k] <=
 * max_outage (the simulation's data window). */
int dvh_outage_first_uncovered(dvh_handle* h, const dvh_outage_case* cases, int32_t count, const int32_t* target_steps,
                               int32_t* first, int32_t* n_uncovered);

/* What is sized for one case.  The case supplies the series, dt, rte, dg_gen, pv_vari and load_shed_pct; its soe0,
 * soe_min, soe_max, charge_max, discharge_max, init_soe and gamma's energy check are the simulation's and are
 * overwritten per candidate (soe0 = soc_init E, soe_min / soe_max = llsoc / ulsoc E, charge_max = discharge_max = P). */
typedef struct dvh_sizing_spec {
  double target_hours;            /* L = round-half-even(target_hours / dt) steps, 1 <= L <= max_outage           */
  int32_t size_energy, size_power; /* at least one; a sized quantity needs a positive unit cost                    */
  double ccost, ccost_kw, ccost_kwh; /* capex = ccost + ccost_kw P + ccost_kwh E                                   */
  double energy_min, energy_max;  /* bounds of a sized E (max: +INFINITY for none)                                 */
  double power_min, power_max;    /* bounds of a sized P                                                           */
  double energy, power;           /* the rating that is not sized                                                  */
  double llsoc, ulsoc, soc_init;  /* fractions                                                                     */
  int32_t n_seed, max_rounds;     /* starts of the first round (>= 1), round limit (1 .. 65536)                    */
} dvh_sizing_spec;

/* The sizing LP of every case over given outage starts, built on the device from the resident series and solved as
 * one batch with the handle's options: per case k over its starts S = starts[sum n_starts[<k] ..] (K = n_starts[k]
 * >= 1 steps of the series) and L steps,
 *   x = [E, P | per window w: ch[0..L-1], dis[0..L-1], s[0..L-1]]  (n = 2 + 3 K L; s_k = energy after step k)
 *   KL equalities (window-major): s_k - s_{k-1} - rte dt ch_k + dt dis_k = 0,  s_{-1} = min(soc_init, ulsoc) E
 *   5 KL >= rows, per (w, k): ulsoc E - s_k >= 0, s_k - llsoc E >= 0, P - ch_k >= 0, P - dis_k >= 0,
 *     dis_k - ch_k >= d,  d = shed_k cl[i] - dg_gen - pv_vari[i], i = t_w + k, shed_k = load_shed_pct[k] / 100 or 1
 *     (d = 0 for i >= n_steps)
 *   min ccost_kwh E + ccost_kw P + ccost;  dispatch columns in [0, inf), a sized E / P in its bounds, else fixed.
 * Bit-identical to dervet_hip/lp/sizing.py sizing_lp (tests/test_gpu_sizing.py).  out[k]: dvh_result of case k (x [n],
 * y [6 K L] caller-allocated or NULL).  Blocks. */
int dvh_sizing_windows(dvh_handle* h, const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count,
                       const int32_t* starts, const int32_t* n_starts, dvh_result* out);

#define DVH_SIZING_SIZED 0
#define DVH_SIZING_ROUND_LIMIT 1 /* max_rounds rounds done; energy / power = the last candidate                     */
#define DVH_SIZING_STALLED 2     /* the scan kept returning a start already in the LP                               */
#define DVH_SIZING_LP_FAILED 3   /* an LP did not come back optimal: lp_status = its dvh_result.status              */
typedef struct dvh_sizing_result {
  double energy, power;           /* kWh, kW (integers unless a lower bound or a fixed rating is not)              */
  double capex;                   /* ccost + ccost_kw power + ccost_kwh energy                                     */
  int32_t status;                 /* DVH_SIZING_*                                                                  */
  int32_t lp_status;              /* status of the case's last LP                                                  */
  int32_t rounds;                 /* LPs solved for this case                                                      */
  int32_t n_starts;               /* outage starts in its last LP                                                  */
  int32_t lp_iters;               /* PDHG iterations summed over its LPs                                           */
  int32_t reserved;
  int32_t* starts;                /* caller-allocated [n_seed + max_rounds] or NULL: those starts                  */
} dvh_sizing_result;

/* The loop, for `count` cases at once.  The series are uploaded once; the outage starts are seeded with the first
 * n_seed indices of a stable descending sort of requirement_t = dt sum_{j<L} cl[t + j] (summed in step order, cut at
 * the series end; :120-122,170-174).  Per round, over the unfinished cases: (1) build and solve the LPs in one batched
 * solve with eps = eps_obj = min(the handle's, 1e-8) (the handle's options are restored); (2) candidate of a sized
 * quantity = ceil(x - delta), delta = 1e-7 max(1, |x|), floored at its lower bound (the reference's integer size
 * variables, ESSSizing.py:83,98, relaxed and rounded up); (3) the candidate's limits written into the device case
 * structs; (4) the scan; (5) first < 0: SIZED; first already among the starts: (3)-(4) once more with ceil(x + delta),
 * STALLED if it still is; else the start is appended.  Host traffic per round: the case structs and descriptors.
 * Blocks; runs on the handle's first device. */
int dvh_size_reliability(dvh_handle* h, const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count,
                         dvh_sizing_result* out);
/* Time of the last dvh_size_reliability call (HIP events, milliseconds); out3 (or NULL) = {LP builds + solves,
 * scans, rounds summed over the cases}. */
int dvh_last_sizing_ms(const dvh_handle* h, double* ms, double* out3);

/* ---- Battery degradation on the device (Battery.py:69-110 through storagevet's BatteryTech degradation, restated in
 * dervet_hip/degradation.py; the one feature that couples a scenario's windows).  Rainflow counting (ASTM E1049-85
 * section 5.4.4 as the `rainflow` package writes it: reversals, three-point stack, leftovers as half cycles) of an SOE
 * profile, each cycle's depth = range / rated energy looked up in the cycle-life table (the first row whose upper limit
 * is >= the depth, the last row above them all), damage = sum of count / cycle life in extraction order.  One wave per
 * profile, the profile in LDS, one lane counting: no floating-point atomics, bit-identical to
 * degradation.cycle_damage and run to run (tests/test_gpu_rainflow.py).  Both calls are asynchronous on `stream` (a
 * hipStream_t; NULL = the handle's stream, i.e. after its solves), wait for nothing and allocate nothing.
 * T above DVH_RAINFLOW_MAX_T (the profile no longer fits a workgroup's LDS) is DVH_ERR_UNSUPPORTED: there is no host
 * fallback.  n_table: 1 .. DVH_RAINFLOW_MAX_TABLE rows, upper ascending.  All pointers are device pointers.
 *
 * dvh_cycle_damage: damage_out[s] = the damage of row s of ene[S][row_stride] (its first T entries, row_stride >= T)
 * with rated energy e_rated[s]; T < 2 gives 0.  The device form of degradation.cycle_damage. */
#define DVH_RAINFLOW_MAX_T 20351
#define DVH_RAINFLOW_MAX_TABLE 64
int dvh_cycle_damage(dvh_handle* h, const double* ene, int64_t row_stride, int32_t S, int32_t T, const double* e_rated,
                     const double* upper, const double* life, int32_t n_table, double* damage_out, void* stream);

/* Degradation state of S batteries, [S] device arrays (dervet_hip.degradation.Degradation's, element for element). */
typedef struct dvh_degradation_state {
  int32_t incl_cycle_degrade;     /* 0: the module is off, calendar loss included (Battery.py:82, :101)             */
  int32_t reserved;
  const double* e_rated;          /* in: rated energy, kWh                                                          */
  const double* yearly;           /* in: calendar degradation, % per year                                           */
  const double* soh;              /* in: state of health at which the battery is worn, fraction of rated            */
  const int32_t* replaceable;     /* in: 1 = reset to nameplate when worn                                           */
  double* degrade_perc;           /* in/out: accumulated degradation, fraction                                      */
  int64_t* replacements;          /* in/out                                                                         */
  int64_t* skipped;               /* in/out: windows whose dispatch was not used                                    */
  double* capacity;               /* out: max(e_rated (1 - degrade_perc), 0) after the update: the next window's E  */
  double* degradation;            /* out: this window's degradation                                                 */
  int32_t* reached;               /* out: 1 = worn in this window (before any replacement)                          */
} dvh_degradation_state;

/* Degradation.update on the device, for the S windows first .. first + S - 1 of a solved packed batch: battery s is
 * updated from window first + s, whose SOE profile is x[off_n + ene_col .. + T - 1] (battery windows: ene_col = 2 T)
 * and whose dispatch counts when istats status is DVH_OPTIMAL.  Per battery, in Degradation.update's operations and
 * order: d = yearly / 100 * (days / 365); a counted window adds cycle damage * (1 - eol_condition / 100), any other
 * takes the calendar loss only and skipped += 1; degrade_perc += d; reached = capacity <= e_rated * soh; a replaceable
 * battery that reached it gets degrade_perc = 0, replacements += 1.  The descriptors live on the device, so a window
 * whose profile does not lie inside it (ene_col + T > n, or the window outside x) is caught there: it is treated as
 * not counted, never read.  incl_cycle_degrade = 0: nothing is updated; degradation = 0, reached = 0 and the unchanged
 * capacity are written.  state->capacity may be handed to dvh_build_battery_group as the next position's E. */
int dvh_degradation_update(dvh_handle* h, const dvh_packed* batch, int32_t first, int32_t S, int32_t T,
                           int32_t ene_col, double days, double eol_condition, const double* upper, const double* life,
                           int32_t n_table, const dvh_degradation_state* state, void* stream);

/* ---- Scenario valuation on the device (dervet/CBA.py:215-233, 299-346, 479-523 on storagevet's Financial, which is
 * absent; restated as far as the Usecase 2 goldens simple_monthly_bill / pro_forma / npv / payback / cost_benefit pin
 * it, dervet_hip/valuation.py): the monthly bill of every solved window, then per scenario the pro forma, its present
 * values, payback and IRR, so that a sweep learns which scenarios are worth building without its dispatch leaving HBM.
 * Both calls are asynchronous on `stream` (a hipStream_t; NULL = the handle's stream, i.e. after its solves), wait for
 * nothing and allocate no device memory (the handle's first call creates its timing events).  No floating-point
 * atomics, fixed-order reductions: bit-identical run to run, and the bill bit-identical to valuation.bill_windows_host.
 * Not restated (zero in every golden; a caller passes them through `extra`): taxes and MACRS, replacement, salvage and
 * decommissioning, ECC.  All pointers are device pointers unless marked host.
 *
 * dvh_bill_windows: the bill of windows first .. first + G - 1 of a solved packed batch, one 256-thread workgroup per
 * window.  x is read through the descriptors in builder.battery_group's layout [ch, dis, ene, tau, pv?, elec?, on?]
 * (has_pv: a curtailable-PV block of T columns after tau; has_ice: elec and on after that); the series are the compact
 * arrays of dvh_battery_group (the same device arrays may be passed) plus `orig`, the site load alone.  Per step
 *   net_t = ((base_t + ch_t) - dis_t) - pv_t - elec_t                       (adds and subtracts only, in this order)
 *   net_t = ((base_t + ch_t) - dis_t) + ev_ch_t                             (has_ev: the EV's charging is net load;
 *                                                                            the "original" rows are unchanged)
 * and bills[g][0 .. DVH_BILL_ROWS - 1] =
 *   [0] retail energy charge  sum_t (retail_t dt) net_t              [5] the same of orig_t (the golden "Original")
 *   [1] demand charge  sum_j demand_j max_{rows i, dcm_j[i] = j} net_{dcm_t[i]}, in j order   [6] the same of orig
 *   [2] DA energy cost  sum_t (da_t dt) net_t                        [7] the same of orig
 *   [3] variable O&M  (om / 1000 dt) sum_t dis_t                     [4] ICE fuel  ice_cost sum_t elec_t
 * (a missing price series bills 0; a tau column without rows bills 0).  The peaks are the dispatch's own, not tau,
 * which is only within solver tolerance of them; peaks (or NULL) [G][J] receives them in kW.  A window whose istats
 * status is not DVH_OPTIMAL, or whose descriptor puts a needed column outside its n or the window outside x, is never
 * read: rows 0 - 4 and its peaks are NaN, rows 5 - 7 are written, and bad[g] = 1 (else 0; + 2 when a demand-charge row
 * named no step or no tau column and was skipped).  J above DVH_BILL_MAX_J is DVH_ERR_UNSUPPORTED. */
#define DVH_BILL_ROWS 8
#define DVH_BILL_MAX_J 16
typedef struct dvh_bill_group {
  int32_t T, J, G, mI;             /* steps, tau columns, windows, demand-charge rows                            */
  double dt;                       /* hours per step                                                             */
  int32_t has_pv, has_ice;         /* column blocks after tau                                                    */
  const int32_t* dcm_t;            /* [mI] step of each demand-charge row                                        */
  const int32_t* dcm_j;            /* [mI] its tau column                                                        */
  const double* base;              /* [G*T] net load + housekeeping power, kW (dvh_battery_group base)           */
  const double* orig;              /* [G*T] site load alone, kW, or NULL: base                                   */
  const double* retail;            /* [G*T] $/kWh or NULL                                                        */
  const double* da;                /* [G*T] $/kWh or NULL                                                        */
  const double* demand;            /* [G*J] $/kW                                                                 */
  const double* om;                /* [G] variable O&M, $/MWh, or NULL: 0                                        */
  const double* ice_cost;          /* [G] $/kW per step (dvh_battery_group ice_cost); has_ice                    */
  int32_t has_ev, pad_ev;          /* an EV block (ev_ch, ev_ene: 2T columns) after tau; not with has_pv / has_ice  */
} dvh_bill_group;
int dvh_bill_windows(dvh_handle* h, const dvh_bill_group* group, const dvh_packed* batch, int32_t first,
                     double* bills, double* peaks, int32_t* bad, void* stream);

/* dvh_value_scenarios: one thread per scenario.  Scenario s owns the CSR entries win_ptr[s] .. win_ptr[s + 1] - 1:
 * win_idx[e] is a row of `bills`, win_year[e] the pro forma year it belongs to (0 = the first year after the CAPEX
 * row), listed in (opt year, window) order -- a seeded sweep packs its seeds first, so a scenario's windows are
 * scattered.  The pro forma has Y + 1 rows (row 0 = the CAPEX year) and C = DVH_CBA_FIXED_COLS + n_extra columns:
 *   [0] -capex[s] in row 0;  [1] avoided energy charge, [2] avoided demand charge, [3] DA value: original - with-DER,
 *   [4] -variable O&M, [5] -fuel: in an opt year the sum over that year's windows in CSR order; a year that is not an
 *   opt year takes the nearest earlier opt year's value times (1 + growth / 100)^(years since), years before the first
 *   opt year are de-escalated from it (one opt year: exactly the golden rows; several: UNPINNED);
 *   [6] -fixed_om[s] in every year, unescalated;  [7 ..] extra[j][0 .. Y] verbatim, shared by the scenarios (the
 *   golden's Tax Credit, Other Incentives, User Constraints Value, or anything DER-VET computes elsewhere).
 * values[s][0 .. DVH_VALUE_COLS - 1] =
 *   [0] lifetime present value  sum_k net_k / (1 + rate)^k, k = 0 at the CAPEX row (numpy's old np.npv)
 *   [1] present-value cost, [2] present-value benefit: each column discounted on its own; one with a negative present
 *       value adds its magnitude to the cost, one with a positive to the benefit (the golden cost_benefit row)
 *   [3] benefit / cost (CBA.py:510-523), NaN when |cost| <= 1e-8.  The golden payback file's "Cost-Benefit Ratio" is
 *       the inverse, from an older reference version: [1] and [2] are what is pinned
 *   [4] payback  capex / net_1 with capex = -net_0;  [5] discounted payback  ln(1 / (1 - capex rate / net_1)) /
 *       ln(1 + rate), NaN when the argument is <= 0 (rate = 0: the payback); both NaN when net_1 <= 0
 *   [6] IRR with np.irr's meaning (CBA.py:498-507): the real rate above -1 at which the NPV is 0, nearest to 0:
 *       bracketed on the grid 1 + rate = (17/16)^i, i = -128 .. 128, outward from rate 0, bisected to 1e-13; NaN when no
 *       grid interval brackets a sign change
 * valid[s] = 0 when any of the scenario's windows is flagged in `bad`, names no row of bills or a year that is not an
 * opt year, when a listed opt year has no window, or when win_ptr (device) is not what win_ptr_host said; else 1.
 * proforma (or NULL) [S][Y + 1][C] receives the full pro forma. */
#define DVH_CBA_MAX_YEARS 64
#define DVH_CBA_MAX_EXTRA 16
#define DVH_CBA_FIXED_COLS 7
#define DVH_VALUE_COLS 7
typedef struct dvh_valuation {
  int32_t S, Y, n_opt, n_extra;    /* scenarios, years after the CAPEX row, opt years, extra columns             */
  int64_t n_win, n_bills;          /* len(win_idx), rows of bills                                                */
  const int32_t* opt_years;        /* host [n_opt] ascending, 0 <= . < Y                                         */
  const int64_t* win_ptr_host;     /* host [S + 1]: validated before the launch                                  */
  const int64_t* win_ptr;          /* [S + 1] the same on the device                                             */
  const int32_t* win_idx;          /* [n_win]                                                                    */
  const int32_t* win_year;         /* [n_win]                                                                    */
  const double* bills;             /* [n_bills][DVH_BILL_ROWS] (dvh_bill_windows)                                */
  const int32_t* bad;              /* [n_bills] its flags, or NULL                                               */
  double rate;                     /* npv discount rate, fraction, > -1                                          */
  double growth[5];                /* %/yr of columns 1 .. 5                                                     */
  const double* capex;             /* [S] $                                                                      */
  const double* fixed_om;          /* [S] $/yr                                                                   */
  const double* extra;             /* [n_extra][Y + 1] $                                                         */
} dvh_valuation;
int dvh_value_scenarios(dvh_handle* h, const dvh_valuation* v, double* values, int32_t* valid, double* proforma,
                        void* stream);
/* Kernel times of the handle's most recent dvh_bill_windows and dvh_value_scenarios (HIP events, milliseconds;
 * 0 for one that has not run): ms2 = {bill, valuation}.  Waits for those two kernels. */
int dvh_last_valuation_ms(const dvh_handle* h, double* ms2);

/* ---- Economic sizing (ESSSizing.py:82-110, ContinuousSizing.sizing_objective, MicrogridScenario.py:208-217, 293-295
 * with the annuity scalar of CBA.py:190-213; restated in dervet_hip/value_sizing.py): the energy and power rating that
 * minimise lifetime cost
 *   F(E, P) = c_energy E + c_power P + c_fixed + alpha sum_w V_w(E, P),
 * V_w the optimum of the case's battery window w (dvh_build_battery_group's LP) at the rating E, pch = pdis = P, and
 * c_energy = ccost_kwh, c_power = ccost_kw + alpha fixedOM, c_fixed = ccost.  Only the window's init / final right-hand
 * sides (soc_target E), its ch / dis upper bounds (P) and its ene bounds (llsoc E, min(ulsoc E, emax_t)) depend on the
 * rating, so V_w is convex and piecewise linear in it, and Kelley's cutting planes size the case: solve the windows at
 * candidate ratings (dvh_solve_packed_device), cut (dvh_value_cuts), solve the master (dvh_value_master), repeat.
 * Deviations from the reference: the integer sizes are relaxed and rounded up afterwards (lp.sizing.candidate), a sized
 * quantity needs a finite box (the master must be bounded), has_ice and has_emin are DVH_ERR_UNSUPPORTED, and the charge
 * and discharge ratings are one sized power: a window whose pch and pdis differ is refused by the cut pass (flag 4).
 *
 * The cut of a solved window at s = (E, P), from its returned y (>= rows clamped at 0): r = c - K'y, and by weak duality
 *   V_w(s') >= D_w(s') = q(s')'y + sum_j [ l_j(s') r_j^+ - u_j(s') r_j^- ] + c0        for every s'
 * (a term whose bound is infinite is dropped; rinf = the largest |r_j| pointing at one).  D_w is convex; linearised at s
 * with the active piece of each ene bound:
 *   g_E = soc_target (y_0 + y_T) + sum_t [ llsoc r_ene,t^+ - ulsoc r_ene,t^- (ulsoc E <= emax_t) ]
 *   g_P = -sum_t (r_ch,t^- + r_dis,t^-),      a = D_w(s) - g_E E - g_P P,      theta_w >= a + g_E E' + g_P P'.
 * The cut holds for any y, so a window that stopped at ITER_LIMIT still yields a valid one.
 *
 * dvh_value_cuts: the cuts of windows first .. first + G - 1 of a solved packed batch built from `group` (the same
 * device arrays), one 256-thread workgroup per window; cuts_out[g][0 .. DVH_VALUE_CUT_COLS - 1] =
 *   {a, g_E, g_P, D_w(s) (dual objective), c'x + c0 (primal objective), rinf, flag, window status, iterations, 0}.
 * K'y is formed from the battery pattern's column structure, every CSR row checked against it on the device, and the
 * demand-charge rows must come period by period with ascending steps (the builder's order); flag != 0 (1: the
 * descriptor is not the group's shape or the window lies outside the arrays, 2: a row is not the pattern's, 4: pch !=
 * pdis): the window was not read and the other columns are NaN.  Windows above 768 steps (the annual hourly window)
 * keep their per-step demand-charge duals in a workspace of the handle, allocated on their first use.  No
 * floating-point atomics, fixed-order reductions: bit-identical run to run, to the host restatement
 * (csrc/dvh_value_cut.h) and whatever else the batch holds.  Asynchronous on `stream` (a hipStream_t; NULL = the
 * handle's stream, i.e. after its solves).  DVH_ERR_UNSUPPORTED: has_ice, has_emin, J above DVH_VALUE_MAX_J. */
#define DVH_VALUE_CUT_COLS 10
#define DVH_VALUE_MAX_J 64
#define DVH_VALUE_MAX_CUTS 256
#define DVH_VALUE_MAX_CAND 8
int dvh_value_cuts(dvh_handle* h, const dvh_battery_group* group, const dvh_packed* batch, int32_t first,
                   double* cuts_out, void* stream);

/* What is sized for one case (a sized quantity: its box, finite; a rating that is not sized: min = max = the rating). */
typedef struct dvh_value_spec {
  int32_t size_energy, size_power; /* at least one                                                                  */
  double c_energy, c_power;        /* $/kWh, $/kW (ccost_kw + alpha fixedOM); > 0 for a sized quantity              */
  double c_fixed;                  /* $                                                                             */
  double alpha;                    /* annuity scalar, > 0                                                           */
  double energy_min, energy_max;   /* kWh                                                                           */
  double power_min, power_max;     /* kW                                                                            */
  double gap_tol;                  /* stop at upper - lower <= gap_tol (1 + |upper|); > 0                           */
  int32_t max_rounds, reserved;    /* 1 .. 65536                                                                    */
} dvh_value_spec;

#define DVH_VALUE_SIZED 0
#define DVH_VALUE_ROUND_LIMIT 1   /* max_rounds rounds done, or the cut list is full                                */
#define DVH_VALUE_LP_FAILED 2     /* a candidate's window did not come back OPTIMAL (e.g. sdr > 0 at P = 0):        */
                                  /* flags[DVH_VF_LP_STATUS] = that window's status, -1 for a flagged cut           */
#define DVH_VALUE_MASTER_FAILED 3 /* the master solve did not end (flags[DVH_VF_MASTER]; not observed)              */
/* state[case][DVH_VALUE_STATE_COLS] (doubles) and flags[case][DVH_VALUE_FLAG_COLS] (int32), device arrays the caller
 * initialises: state = {-inf, +inf, 0, ...}, flags = 0. */
#define DVH_VALUE_STATE_COLS 8
#define DVH_VS_LOWER 0  /* best master optimum + c_fixed                                                            */
#define DVH_VS_UPPER 1  /* best F at a candidate, from the windows' primal objectives                               */
#define DVH_VS_INC_E 2  /* the incumbent: the candidate of `upper`                                                  */
#define DVH_VS_INC_P 3
#define DVH_VS_INC_V 4  /* its sum_w V_w                                                                            */
#define DVH_VS_Z_E 5    /* the last master optimum                                                                  */
#define DVH_VS_Z_P 6
#define DVH_VS_THETA 7
#define DVH_VALUE_FLAG_COLS 8
#define DVH_VF_DONE 0
#define DVH_VF_STATUS 1
#define DVH_VF_LP_STATUS 2
#define DVH_VF_NCUTS 3
#define DVH_VF_ROUNDS 4
#define DVH_VF_LP_ITERS 5
#define DVH_VF_MASTER 6

/* One round's master step for `count` cases, one wave per case.  Case k of the call is case case_ids[k] of the
 * n_cases the per-case arrays hold; its windows were solved at n_cand candidates, and window_cuts[p][k][j][.] is
 * dvh_value_cuts' record of window position p (W positions) of candidate j, whose rating is E_in / P_in [k][j].  Per
 * case: the candidates' cuts summed over the positions in position order and appended to cuts[case][.][3] (cut_cap
 * rows, <= DVH_VALUE_MAX_CUTS); upper / the incumbent updated from F at each candidate; the master
 *   min c_energy E + c_power P + alpha theta   s.t.  theta >= a_k + gE_k E + gP_k P,  E, P in their boxes
 * solved exactly (a dual simplex on three-constraint bases, deterministic); lower = max(lower, its optimum + c_fixed);
 * done with DVH_VALUE_SIZED when upper - lower <= gap_tol (1 + |upper|), with DVH_VALUE_ROUND_LIMIT after max_rounds
 * rounds or when the next round's cuts would not fit, with DVH_VALUE_LP_FAILED when a candidate's window is not
 * OPTIMAL; else the next round's n_next candidates -- the master optimum z*, then inc + (j / n_next)(z* - inc),
 * j = 1 .. n_next - 1, inc the incumbent -- written to E_out / pch_out / pdis_out [k][j], the arrays the builder reads
 * (they may be E_in / P_in themselves only when n_next = n_cand).  A case already done is left as it is.
 * spec_host is validated before the launch and must equal the device copy `spec`.  Asynchronous on `stream`. */
typedef struct dvh_value_master_args {
  int32_t count, n_cases, W, n_cand, n_next, cut_cap;
  const dvh_value_spec* spec_host; /* host [n_cases]                                                                */
  const dvh_value_spec* spec;      /* [n_cases] the same on the device                                              */
  const int32_t* case_ids;         /* [count]                                                                       */
  const double* window_cuts;       /* [W][count][n_cand][DVH_VALUE_CUT_COLS]                                        */
  const double* E_in;              /* [count][n_cand]                                                               */
  const double* P_in;              /* [count][n_cand]                                                               */
  double* cuts;                    /* [n_cases][cut_cap][3]                                                         */
  double* state;                   /* [n_cases][DVH_VALUE_STATE_COLS]                                               */
  int32_t* flags;                  /* [n_cases][DVH_VALUE_FLAG_COLS]                                                */
  double* E_out;                   /* [count][n_next]                                                               */
  double* pch_out;                 /* [count][n_next]                                                               */
  double* pdis_out;                /* [count][n_next]                                                               */
} dvh_value_master_args;
int dvh_value_master(dvh_handle* h, const dvh_value_master_args* args, void* stream);

/* Kernel cascade (testing / A-B timing): 0 = default (battery-banded -> ELL -> generic CSR), 1 = generic
 * CSR kernel for every window, 2 = ELL -> generic (no battery-banded kernel), 3 / 4 = as 0 with the battery-banded
 * kernel's form forced: one step per lane (768 threads per window, one window per CU) / three steps per lane (256
 * threads, two windows per CU).  The default picks the one-step form when the batch has at most one battery window
 * per compute unit, else the three-step form.  5 = as 0 plus the band kernel's interconnection form (opt-in): battery
 * windows with POI import / export limit rows, a curtailable-PV column block (x = [ch, dis, ene, tau, pv]) and / or
 * charge-from-PV rows (PV grid_charge = 0), which the default cascade hands down to the generic CSR kernel, are
 * taken after the ICE pass by a 768-thread kernel of their own and counted as band windows; every other window lands
 * where mode 0 puts it, and the mode adds no host wait.  6 = as 0 plus the band kernel's load-shift form (opt-in):
 * battery windows with a controllable load (x = [ch, dis, ene, tau, pw, el], the battery's T + 1 equality rows followed
 * by the load's T + D: per day the day-start row, the el recurrence and the day-end row; every DCM row may carry
 * pw_t), which mode 0 leaves to the ELL / generic kernels, are taken after the ICE pass by a 768-thread kernel of
 * their own and counted as band windows, as mode 5 does for its windows; dvh_options.kkt_predict is ignored by that
 * kernel and certify works through the after-pass.  One form is added at a time: mode 6 does not run mode 5's.
 * 7 = as 0 plus the band kernel's heat form (opt-in): battery windows with one combined-heat-and-power unit
 * (x = [ch, dis, ene, tau, elec, on, steam, hotwater], the battery's T + 1 equality rows followed by T heat rows
 * (elec_t, steam_t, hotwater_t; right-hand side 0); among the >= rows, besides the DCM rows (which may carry elec_t),
 * per step two generator rows (elec_t, on_t) and one ratio row (steam_t, hotwater_t), right-hand sides 0; 0 <= elec,
 * 0 <= on <= a finite bound at no cost, steam and hotwater bounded below only), which mode 0 leaves to the ELL / generic
 * kernels and, from n or m > 4096 on (T >= 586), to the grid-wide path one window at a time, are taken by a 768-thread
 * kernel of their own (T <= 768) and counted as band windows; the windows up to 4096 after the ICE pass without a host
 * wait, as modes 5 and 6, the larger ones behind their chunk's tiers with one status read-back per batch.
 * dvh_options.kkt_predict is ignored by that kernel and certify works through the after-pass (up to 4096). */
int dvh_set_kernel_path(dvh_handle* h, int mode);

/* Launch order of the next solve (scheduling only: the results do not depend on it).  order: host array, a
 * permutation of 0 .. count - 1 (validated; DVH_ERR_ARG otherwise), copied.  The next dvh_solve_packed_device /
 * dvh_solve_batch launches its battery-band pass over the windows in this order when count equals its window count
 * and the batch is one chunk of on-chip windows (else the packing order); the order is consumed by that solve.
 * Longest-expected-first orders shorten the launch's tail (dervet_hip/sweep.py orders a warm phase by its seeds'
 * iteration counts).  count 0 clears. */
int dvh_set_launch_order(dvh_handle* h, const int32_t* order, int32_t count);

#ifdef __cplusplus
}
#endif
#endif /* DERVET_HIP_H */
