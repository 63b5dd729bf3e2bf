"""The LPs of tests/test_gpu_planted.py and tests/test_gpu_result_contract.py, with the kernel each must reach.
tests/test_planted_lp.py checks on the CPU that every one of them has the planted optimum (HiGHS) and that the host
restatement of the algorithm (oracle/pdlp_ref.py) solves it in at most 25,000 of the default 100,000 iterations, so no
GPU tier can excuse a failure by "hard instance".  Seeds are fixed here; no case is left out at run time.

How the shapes follow from the dispatch (csrc/dvh_kernels.hip launch_pdhg_ell, small_dispatch, ell_dispatch_xy;
csrc/dvh_cascade.cpp device_cascade):
  * the route kernel splits the windows that reach the ELL kernels in two classes, n <= 512 and m <= 768, and the rest;
    each class is sized by its largest n and m and by wx / wy, the widest column / row among those of at most 8
    entries (longer ones are "long" and do not count);
  * latency = the class has at most two windows per CU;
  * small kernels (class 1, wx <= 6, wy <= 8): <256,1,2> for n <= 256, m <= 512; <256,2,2> for n, m <= 512, skipped
    when latency and wx <= 4; <256,2,3> for m <= 768 when wx > 4;
  * otherwise the <2,4> slices for wx <= 2 and wy <= 4, else the <4,8> slices for wx <= 4: <512,1,1>, <512,2,2>,
    <768,3,2> (<2,4> only), <512,5,3> (<2,4> only: its <4,8> form does not fit the LDS and is not compiled);
  * anything else takes the generic CSR kernel, sized xs = ceil(n / 512), ys = ceil(m / 512), with K and K' in LDS when
    pdhg_lds_bytes(n, m, nnz, true) <= 160 KiB (generic_lds_bytes below restates it for the CPU check).
The variant code of an ELL instantiation is (2 + KR) 10^6 + WX 10^5 + WY 10^4 + (B / 64) 100 + 10 X + Y, of the generic
kernel 1000 (matrices in LDS) + 10 xs + ys.
"""
import functools

import numpy as np

import band_cases
import planted_lp

# name -> (n, m_eq, m_ineq, wy, wx, seed, options, path, copies, tier, variant, distance check)
#   tier: the kernel_stats count that must equal the batch ("ell_windows", "generic_windows", "large_windows"), or
#   None: ELL or generic (the ELL kernels may hand a window with long rows on)
#   distance check: False where the host reference itself misses 1e-4 (1 + |x*|) / (1 + |y*|) (test_planted_lp prints
#   its distances): the scale-spread windows, whose duals span four decades
_E, _G, _L = "ell_windows", "generic_windows", "large_windows"
GENERAL = {
    # ---- the small ELL kernels
    "small12_at": (256, 200, 312, 8, 6, 1, {}, "default", 1, _E, 5680412, True),
    "small12_below": (255, 150, 361, 4, 4, 1, {}, "default", 1, _E, 5680412, True),
    "small22_at": (512, 200, 312, 8, 6, 1, {}, "default", 1, _E, 5680422, True),
    "small22_n257": (257, 150, 362, 8, 5, 1, {}, "default", 1, _E, 5680422, True),
    "small22_many": (257, 100, 100, 4, 2, 1, {}, "default", 520, _E, 5680422, True),  # latency = false
    "small23_at": (512, 300, 468, 8, 6, 1, {}, "default", 1, _E, 2680423, True),
    "small23_m513": (256, 100, 413, 8, 5, 1, {}, "default", 1, _E, 2680423, True),
    "small12_spread": (255, 100, 150, 8, 6, 1, dict(scale_spread=2.0), "default", 1, _E, 5680412, False),
    "small12_empty": (200, 60, 90, 4, 4, 1, dict(empty_cols=3, empty_rows=3), "default", 1, _E, 5680412, True),
    "small22_long": (300, 100, 150, 6, 6, 1, dict(long_rows=3, long_row_len=40, long_cols=2, long_col_len=12),
                     "default", 1, None, 5680422, True),
    # ---- the <2,4> slices
    "ell24_11_at": (512, 200, 312, 4, 2, 1, {}, "default", 1, _E, 5240811, True),
    "ell24_11_below": (511, 150, 250, 4, 2, 1, {}, "default", 1, _E, 5240811, True),
    "ell24_22_at": (1024, 400, 624, 4, 2, 1, {}, "default", 1, _E, 5240822, True),
    "ell24_22_n513": (513, 150, 250, 4, 2, 1, {}, "default", 1, _E, 5240822, True),
    "ell24_32_at": (2304, 700, 836, 4, 2, 1, {}, "default", 1, _E, 5241232, True),
    "ell24_32_n1025": (1025, 300, 500, 4, 2, 1, {}, "default", 1, _E, 5241232, True),
    "ell24_53_at": (2560, 700, 836, 4, 2, 1, {}, "default", 1, _E, 2240853, True),
    "ell24_53_n2305": (2305, 600, 700, 4, 2, 1, {}, "default", 1, _E, 2240853, True),
    "ell24_n2561": (2561, 600, 700, 4, 2, 1, {}, "default", 1, _G, 1063, True),  # one above: no ELL holds it
    # ---- the <4,8> slices
    "ell48_11_at": (512, 200, 312, 8, 4, 1, {}, "default", 1, _E, 5480811, True),
    "ell48_11_wx3": (300, 100, 157, 4, 3, 1, {}, "default", 1, _E, 5480811, True),
    "ell48_11_wy5": (300, 60, 60, 5, 2, 1, {}, "default", 1, _E, 5480811, True),
    "ell48_22_at": (1024, 400, 624, 8, 4, 1, {}, "default", 1, _E, 5480822, True),
    "ell48_n1025": (1025, 400, 600, 8, 4, 1, {}, "default", 1, _G, 1032, True),  # one above: <4,8> has no wider form
    "ell_wx5_n600": (600, 200, 300, 8, 5, 1, {}, "default", 1, _G, 1021, True),  # one above WX = 4 past the small kernels
    "ell_wx7": (200, 80, 100, 8, 7, 1, {}, "default", 1, _G, 1011, True),  # one above the small kernels' WX = 6
    # ---- the generic kernel's five sizes, matrices in LDS and not
    "gen22_lds": (1024, 400, 624, 4, 4, 1, {}, "generic", 1, _G, 1022, True),
    "gen22": (1023, 400, 623, 8, 8, 1, {}, "generic", 1, _G, 22, True),
    "gen53_lds": (2560, 700, 836, 3, 3, 1, {}, "generic", 1, _G, 1053, True),
    "gen53": (2559, 700, 835, 4, 4, 1, {}, "generic", 1, _G, 53, True),
    "gen64_lds": (3072, 900, 1148, 2, 2, 1, {}, "generic", 1, _G, 1064, True),
    "gen64": (3071, 900, 1147, 3, 3, 1, {}, "generic", 1, _G, 64, True),
    "gen66_lds": (3072, 1300, 1772, 1, 1, 1, {}, "generic", 1, _G, 1066, True),
    "gen66": (3071, 1300, 1771, 2, 2, 1, {}, "generic", 1, _G, 66, True),
    # (8, 8) with the matrices in LDS needs fewer entries than columns: empty columns and empty >= rows
    "gen88_lds": (3600, 2000, 1600, 1, 1, 1, dict(empty_cols=500, empty_rows=500), "generic", 1, _G, 1088, True),
    "gen88": (4096, 1500, 2596, 2, 2, 1, {}, "generic", 1, _G, 88, True),
    "gen_rows_32_33": (600, 200, 250, 6, 6, 1, dict(long_rows=2, long_row_len=(32, 33), long_cols=2,
                                                    long_col_len=(32, 33)), "generic", 1, _G, 1021, True),
    "gen_long64": (1200, 400, 500, 4, 4, 1, dict(long_rows=64, long_row_len=33), "generic", 1, _G, 1032, True),
    # ---- the row side of every instantiation: m one below its Y B slots, and one above, which hands the window on
    "small12_m513": (256, 100, 413, 4, 4, 1, {}, "default", 1, _E, 5480822, True),  # wx <= 4: past <256,1,2> to <4,8>
    "small22_m511": (512, 200, 311, 8, 6, 1, {}, "default", 1, _E, 5680422, True),
    "small22_m513": (512, 200, 313, 8, 6, 1, {}, "default", 1, _E, 2680423, True),
    "small22_n513": (513, 200, 300, 8, 6, 1, {}, "default", 1, _G, 1021, True),  # wx = 6 past the small kernels' n
    "small23_m767": (512, 300, 467, 8, 6, 1, {}, "default", 1, _E, 2680423, True),
    "small23_m769": (512, 300, 469, 8, 6, 1, {}, "default", 1, _G, 1012, True),
    "small23_n511": (511, 300, 400, 8, 5, 1, {}, "default", 1, _E, 2680423, True),
    "ell24_11_m511": (512, 200, 311, 4, 2, 1, {}, "default", 1, _E, 5240811, True),
    "ell24_11_m513": (512, 200, 313, 4, 2, 1, {}, "default", 1, _E, 5240822, True),
    "ell24_22_m1023": (1024, 400, 623, 4, 2, 1, {}, "default", 1, _E, 5240822, True),
    "ell24_22_m1025": (1024, 400, 625, 4, 2, 1, {}, "default", 1, _E, 5241232, True),
    "ell24_32_m1535": (2304, 700, 835, 4, 2, 1, {}, "default", 1, _E, 5241232, True),
    "ell24_32_m1537": (2304, 700, 837, 4, 2, 1, {}, "default", 1, _G, 1054, True),  # <512,5,3> holds 1536 rows too
    "ell24_53_m1535": (2560, 700, 835, 4, 2, 1, {}, "default", 1, _E, 2240853, True),
    "ell24_53_m1537": (2560, 700, 837, 4, 2, 1, {}, "default", 1, _G, 1054, True),
    "ell48_11_m511": (512, 200, 311, 8, 4, 1, {}, "default", 1, _E, 5480811, True),
    "ell48_11_m513": (512, 200, 313, 8, 4, 1, {}, "default", 1, _E, 5480822, True),
    "ell48_22_m1023": (1024, 400, 623, 8, 4, 1, {}, "default", 1, _E, 5480822, True),
    "ell48_22_m1025": (1024, 400, 625, 8, 4, 1, {}, "default", 1, _G, 1023, True),
    "gen22_m1025": (1024, 400, 625, 4, 4, 1, {}, "generic", 1, _G, 1023, True),
    "gen22_n1025": (1025, 400, 600, 4, 4, 1, {}, "generic", 1, _G, 1032, True),
    "gen53_m1537": (2560, 700, 837, 3, 3, 1, {}, "generic", 1, _G, 1054, True),
    "gen53_n2561": (2561, 700, 800, 3, 3, 1, {}, "generic", 1, _G, 1063, True),
    "gen64_m2049": (3072, 900, 1149, 2, 2, 1, {}, "generic", 1, _G, 1065, True),
    "gen64_n3073": (3073, 900, 1100, 3, 2, 1, {}, "generic", 1, _G, 74, True),
    "gen66_m3073": (3072, 1300, 1773, 2, 2, 1, {}, "generic", 1, _G, 67, True),
    "gen88_m4095": (4095, 1500, 2595, 2, 2, 1, {}, "generic", 1, _G, 88, True),
    "large_m4097": (4096, 1500, 2597, 2, 2, 1, {}, "default", 1, _L, None, True),  # one row past (8, 8)
    # ---- the set-up kernel's fall-back for m + n > 16 (n + 1) (the long-row flags no longer fit its LDS cursors): few
    # columns, many >= rows; the columns hold up to 20 entries (wx = 20 here bounds them; none counts as an ELL width)
    "setup_many_rows": (40, 10, 690, 1, 20, 1, {}, "generic", 1, _G, 1012, True),
    # ---- the grid-wide path: n = 4097 is past the on-chip kernels and no battery window, so the chain plan refuses it
    "large4097": (4097, 1500, 2000, 4, 4, 1, dict(long_rows=3, long_row_len=40, long_cols=3, long_col_len=40),
                  "default", 1, _L, None, True),
}
# 65 long rows: one more than the on-chip lists hold -- must come back NUMERICAL (no CPU condition: it is not solved)
LONG65 = (1200, 400, 500, 4, 4, 1, dict(long_rows=65, long_row_len=33))
# one window of each size class for the mixed batch (with battery windows): every one keeps the kernel it has alone
MIXED = ("small12_below", "ell24_22_n513", "large4097")


@functools.lru_cache(maxsize=None)
def general(name):
    n, m_eq, m_ineq, wy, wx, seed, opts = GENERAL[name][:7]
    return planted_lp.planted(n, m_eq, m_ineq, wy, wx, seed, **opts)


@functools.lru_cache(maxsize=None)
def long65():
    n, m_eq, m_ineq, wy, wx, seed, opts = LONG65
    return planted_lp.planted(n, m_eq, m_ineq, wy, wx, seed, **opts)


def generic_lds_bytes(n, m, nnz):
    """csrc/dvh_kernels.hip pdhg_lds_bytes(n, m, nnz, true, 8) restated (kNRed = 11 reduced values, kLMax = 64)."""
    a16 = lambda v: (v + 15) // 16 * 16
    return a16(8 * (n + m + 11 * 9 + 640)) + a16(4 * 128) + a16(16 * nnz) + a16(4 * (n + m + 2)) + a16(4 * nnz)


# ---------------------------------------------------------------------------------------------------------------
# the band, ICE, interconnection and chain forms: one realistic window and one planted window (planted_window: the
# realistic window's K, l, u, m_eq with c and q replaced) per shape
BAND_T = (2, 25, 200, 745, 768)
BAND_J = (0, 1, 4)
ICE_PLANT = dict(interior_frac=0.1, active_frac=0.1)  # (at 0.4 the host reference needs 50,000-80,000 iterations)


def battery_window(T, J, seed=5, span=False):
    """band_cases' battery + DCM window; span: the one demand period covers the middle half of the window (both
    segments of a two-segment chain window)."""
    masks = None
    if span and J == 1:
        masks = np.zeros((1, T), bool)
        masks[0, T // 4: 3 * T // 4] = True
    return band_cases.window(T, J, seed, masks=masks)[0]


@functools.lru_cache(maxsize=None)
def band_windows():
    """{name: (realistic oracle dict, planted oracle dict)} over BAND_T x BAND_J."""
    out = {}
    for T in BAND_T:
        for J in BAND_J:
            if J <= T:
                base = planted_lp.from_window(battery_window(T, J))
                out[f"T{T}J{J}"] = (base, planted_lp.planted_window(base, 1))
    return out


@functools.lru_cache(maxsize=None)
def ice_windows():
    from dervet_hip.lp import builder, scenarios
    lps = [lp for g in scenarios.config5(range(2), years=1) for lp in builder.group_window_lps(g)]
    out = {}
    for k in (0, 17):
        base = planted_lp.from_window(lps[k])
        out[f"ice{k}"] = (base, planted_lp.planted_window(base, 1, **ICE_PLANT))
    return out


IC_VARIANTS = ("poi", "poi_pv", "gc_pv", "poi_gc_pv")
INTERCONNECT = tuple((T, J, v) for v in IC_VARIANTS for T, J in ((25, 1), (745, 4)))


@functools.lru_cache(maxsize=None)
def interconnect_windows():
    """test_gpu_interconnect's POI / curtailable-PV / charge-from-PV windows."""
    from dervet_hip.lp import builder
    bat = dict(E=2000.0, Pch=500.0, Pdis=500.0, rte=0.9, sdr=0.0, soc_target=0.5, ulsoc=1.0, llsoc=0.1, fixedOM=1.0,
               OMexpenses=0.0, hp=0.0)
    out = {}
    for T, J, v in INTERCONNECT:
        rng = np.random.default_rng(1000 * T + 10 * J + IC_VARIANTS.index(v))
        t = np.arange(T)
        kw = {}
        if "poi" in v:
            kw["poi"] = dict(max_import=-650.0, max_export=0.0)
        if "pv" in v:
            kw["pv_curtail_max"] = (50.0 + 900.0 * np.sin(np.pi * (t + 0.5) / T))[None]
        if "gc" in v:
            kw["grid_charge"] = False
        masks = np.array([t % (J + 1) == j for j in range(J)], bool).reshape(J, T)
        g = builder.battery_group(T, 1.0, rng.uniform(400.0, 700.0, (1, T)), bat,
                                  retail_price=rng.uniform(0.05, 0.15, (1, T)), demand_masks=masks,
                                  demand_prices=rng.uniform(8.0, 20.0, (1, J)), **kw)
        base = planted_lp.from_window(builder.group_window_lps(g)[0])
        out[f"{v}_T{T}J{J}"] = (base, planted_lp.planted_window(base, 1))
    return out


# 3 T + J > 4096: the chain team.  J = 0: two segments.  J = 1: the demand period, steps [350, 1050), gets a segment of
# its own (the plan's run_cut), so three segments and no shared column; CHAIN_PLAN below holds the windows that share
CHAIN = ((1400, 0), (1400, 1))


@functools.lru_cache(maxsize=None)
def chain_windows():
    out = {}
    for T, J in CHAIN:
        base = planted_lp.from_window(battery_window(T, J, span=True))
        out[f"chainT{T}J{J}"] = (base, planted_lp.planted_window(base, 1))
    return out


# ---- the chain team's plan (csrc/dvh_chain.hip chain_plan_kernel, restated in tests/chain_plan_ref.py): one window per
# branch of the plan and of what the team kernel does with it.
# name -> (T, J, tau id per step (-1: no demand row), the plan's segment starts or None where the plan refuses the
# window, the (slot, other sharer) pairs of every segment, what the case reaches).  The plans are derived by hand from
# the kernel source; tests/test_chain_plan_ref.py holds the restatement to them.  No GPU test solves these windows
# yet, and none may solve s65_J2 before the plan refuses it: its 128 pairs are one more than a segment's poll lists
# hold (tests/chain_plan_ref.py).


def _pieces(T, *pieces):
    """tau ids from (start, id) pieces, each running to the next piece's start; id "tN" = t % N."""
    t = np.arange(T)
    out = np.full(T, -1, np.int64)
    for (a, j), (e, _) in zip(pieces, pieces[1:] + ((T, None),)):
        out[a:e] = t[a:e] % int(j[1:]) if isinstance(j, str) else j
    return out


def _peak(T, other):
    """dt = 0.25: hours 12-17 of each day (steps 48 .. 71 of 96) are column 0, the rest `other`."""
    hour = (np.arange(T) % 96) // 4
    return np.where((hour >= 12) & (hour < 18), 0, other)


def _full(T):
    return tuple(range(0, T, 768)) + (T,)


CHAIN_PLAN = {
    "min_J0": (1366, 0, _pieces(1366, (0, -1)), (0, 768, 1366), 0, "smallest chain window: 3 T > 4096"),
    "route_J2": (1365, 2, _pieces(1365, (0, "t2")), (0, 768, 1365), 2, "n = 4097: the chain, next to its on-chip twin"),
    "all_J1": (1400, 1, _pieces(1400, (0, 0)), (0, 768, 1400), 1, "one shared column"),
    "all_J2": (1400, 2, _pieces(1400, (0, "t2")), (0, 768, 1400), 2, "nsl > 1"),
    "all_J4": (1400, 4, _pieces(1400, (0, "t4")), (0, 768, 1400), 4, "all four slots shared"),
    "five_J5": (1400, 5, _pieces(1400, (0, "t5")), None, None, "refused: 4-step segments until kPMax"),
    "full_J1": (1536, 1, _pieces(1536, (0, 0)), (0, 768, 1536), 1, "lane 767 is the last step of both segments"),
    "tail1_J1": (1537, 1, _pieces(1537, (0, 0)), (0, 768, 1536, 1537), 2, "one-step last segment sharing a column"),
    "tail64_J1": (1600, 1, _pieces(1600, (0, 0)), (0, 768, 1536, 1600), 2, "last segment of 64 steps: wl = 0"),
    "tail65_J1": (1601, 1, _pieces(1601, (0, 0)), (0, 768, 1536, 1601), 2, "last segment of 65 steps: wl = 1"),
    "mid1_J3": (2305, 3, _pieces(2305, (0, -1), (767, 0), (1535, 1), (1536, 2), (2304, 1)),
                (0, 767, 1535, 1536, 2304, 2305), (0, 0, 2, 2, 2),
                "one-step middle and last segments; segment 3 holds column 1 in a free slot"),
    "free_J2": (2304, 2, _pieces(2304, (0, 1), (768, 0), (1536, 1)), (0, 768, 1536, 2304), 2,
                "free-slot sharer with zero partials"),
    "nofree_J5": (2304, 5, _pieces(2304, (0, 4), (768, "t4"), (1536, 4)), None, None, "refused: no free slot"),
    "qh_peak_J2": (2976, 2, _peak(2976, 1), (0, 744, 1512, 2280, 2976), 6, "two-period tariff; run_cut starts"),
    "qh_peak_J1": (2976, 1, _peak(2976, -1), (0, 744, 1512, 2280, 2976), 3, "shared column, steps without a row"),
    "s64_J1": (49152, 1, _pieces(49152, (0, 0)), _full(49152), 63, "DPP tau_total with all 64 lanes; long set-up"),
    "s65_J1": (49920, 1, _pieces(49920, (0, 0)), _full(49920), 64, "sequential tau_total branch"),
    "s64_J2": (49152, 2, _pieces(49152, (0, "t2")), _full(49152), 126, "K list at 254 of 256 entries"),
    "s65_J2": (49920, 2, _pieces(49920, (0, "t2")), _full(49920), 128, "one pair past the poll lists, and planned"),
}
CHAIN_PLAN_LONG = tuple(n for n in CHAIN_PLAN if n.startswith("s6"))  # the 49k windows: the planted twin only
CHAIN_PLAN_OVERFLOW = ("s65_J2",)  # planned with more pairs than the team kernel's poll lists hold
ROUTE_TWIN = (1365, 1)  # route_J2's on-chip twin: n = 4096 stays with the on-chip kernels


@functools.lru_cache(maxsize=None)
def chain_plan_window(name, seed=5):
    """(realistic oracle dict, planted oracle dict) of a CHAIN_PLAN case."""
    T, J, tau = CHAIN_PLAN[name][:3]
    masks = np.array([tau == j for j in range(J)], bool).reshape(J, T) if J else None
    base = planted_lp.from_window(band_cases.window(T, J, seed, masks=masks)[0])
    return base, planted_lp.planted_window(base, 1)


@functools.lru_cache(maxsize=None)
def route_twin():
    T, J = ROUTE_TWIN
    return planted_lp.from_window(band_cases.window(T, J, 5, masks=np.ones((J, T), bool))[0])


def all_window_cases():
    out = {}
    for f in (band_windows, ice_windows, interconnect_windows, chain_windows):
        out.update(f())
    return out
