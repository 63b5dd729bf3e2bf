"""One electric vehicle (dervet MicrogridDER/ElectricVehicles.py ElectricVehicle1, LP mode) on a plain battery window:
the reference's own rows restated densely and independently of dervet_hip.lp.builder, the load-shift kernel's set-up
check restated for the CPU, and the windows the EV tests share (tests/ctrl_load_ref.py's battery and series, 50 kW).

  x = [ch(T), dis(T), ene(T), tau(J), ev_ch(T), ev_ene(T)]          ev_ene free, as in the reference
  ev_ene_a = 0 at every plug-in step a, step 0 included if plugged there                       (:249, :256-257)
  ev_ene_i - ev_ene_{i-1} - dt ev_ch_{i-1} = 0 for every plugged step i > 0                    (:258-262)
  ene_target - ev_ene_{p-1} - dt ev_ch_{p-1} = 0 and ev_ene_p = ene_target at every plug-out step p  (:270-278)
  0 <= ev_ch <= ch_max, ev_ch <= 0 when not plugged                                            (:287-291)
  net load: load_t + ch_t - dis_t + ev_ch_t (get_charge, :135-144)
A plug-in / plug-out step is the first step of / after a maximal plugged run: with dt = 1 h that is the reference's
calendar test (hour == plugin_time / plugout_time), except that a window whose first step is a plug-out hour pins
ev_ene_0 there, which touches no other variable.
"""
import numpy as np
import scipy.sparse as sp

import ctrl_load_ref as cl
from dervet_hip.lp import builder

BAT = cl.BAT
CH_MAX = 50.0


def hours(T, plugin, plugout):
    h = np.arange(T) % 24
    return (h >= plugin) & (h < plugout) if plugin < plugout else (h >= plugin) | (h < plugout)


def _mask(T, on):
    m = np.zeros(T, bool)
    m[list(on)] = True
    return m


# (T, J, plugged, ene_target): the smallest case, one whole session; a leading partial and a trailing cut session
# without DCM; a session wholly inside wave 0 behind a leading unplugged run; a trailing cut session across the wave
# boundary (with a whole session before it: a window without any plug-out step is refused, as the reference fails on
# it); hours 18 -> 7 with negative prices on the trailing session; idle lanes; four demand periods; every lane busy
SHAPES = [(5, 1, _mask(5, [1, 2]), 80.0), (8, 0, _mask(8, [0, 1, 2, 5, 6, 7]), 120.0),
          (64, 1, _mask(64, [60, 61, 62]), 100.0), (65, 4, _mask(65, [20, 21, 22, 62, 63, 64]), 100.0),
          (72, 1, hours(72, 18, 7), 120.0), (129, 1, hours(129, 18, 7), 120.0), (744, 4, hours(744, 18, 7), 200.0),
          (768, 1, hours(768, 9, 17), 200.0)]
IDS = [f"T{s[0]}J{s[1]}" for s in SHAPES]


def series(T, J, G=2):
    load, retail, masks, dprice = cl.series(T, J, G)
    if T == 72:  # negative prices on the trailing session: it charges, as the reference's does
        retail = retail.copy()
        retail[:, 66:] -= 0.2
    return load, retail, masks, dprice


def group(T, J, plugged, target, G=2, ch_max=CH_MAX, fixed_om=3.0):
    load, retail, masks, dprice = series(T, J, G)
    ev = None if ch_max is None else dict(ch_max=ch_max, ene_target=target, fixed_om=fixed_om, plugged=plugged)
    return builder.battery_group(T, 1.0, load, BAT, retail_price=retail, demand_masks=masks, demand_prices=dprice, ev=ev)


def dense_of(T, J, plugged, target, k, G=2, ch_max=CH_MAX, fixed_om=3.0):
    load, retail, masks, dprice = series(T, J, G)
    return dense(T, 1.0, load[k], BAT, retail[k], masks, None if dprice is None else dprice[k], ch_max, target,
                 fixed_om, plugged)


def plug_steps(plugged):
    """(plug-in steps, plug-out steps inside the window) of a mask."""
    pl = np.asarray(plugged, bool)
    prev = np.concatenate([[False], pl[:-1]])
    return np.nonzero(pl & ~prev)[0], np.nonzero(~pl & prev)[0]


def dense(T, dt, load, bat, retail, masks, dprice, ch_max, target, fixed_om, plugged):
    """One window (load, retail [T]; dprice [J]) as an oracle dict: K (csr), q, c, c0, l, u, m_eq."""
    masks = np.zeros((0, T), bool) if masks is None else np.asarray(masks, bool)
    pl = np.asarray(plugged, bool)
    J = len(masks)
    n = 5 * T + J
    ch, dis, ene, tau, ec, ee = 0, T, 2 * T, 3 * T, 3 * T + J, 4 * T + J
    E, eta, sdr = bat["E"], bat["rte"], bat["sdr"] / 100.0
    soc = bat["soc_target"] * E
    rows, q = [], []

    def row(entries, rhs):
        r = np.zeros(n)
        for j, v in entries:
            r[j] += v
        rows.append(r)
        q.append(rhs)

    row([(ene, 1.0)], soc)
    for t in range(T - 1):
        row([(ene + t + 1, 1.0), (ene + t, -(1.0 - dt * sdr)), (ch + t, -dt * eta), (dis + t, dt)], 0.0)
    k = T - 1
    row([(ene + k, 1.0 - dt * sdr), (ch + k, dt * eta), (dis + k, -dt)], soc)
    plug_in, plug_out = plug_steps(pl)
    for a in plug_in:
        row([(ee + a, 1.0)], 0.0)
    for i in np.nonzero(pl)[0]:
        if i > 0:
            row([(ee + i, 1.0), (ee + i - 1, -1.0), (ec + i - 1, -dt)], 0.0)
    for p in plug_out:
        row([(ee + p - 1, -1.0), (ec + p - 1, -dt)], -target)
        row([(ee + p, 1.0)], target)
    m_eq = len(rows)
    base = np.asarray(load, np.float64) + bat.get("hp", 0.0)
    for j in range(J):
        for t in np.nonzero(masks[j])[0]:  # tau_j >= base + ch - dis + ev_ch
            row([(tau + j, 1.0), (ch + t, -1.0), (dis + t, 1.0), (ec + t, -1.0)], base[t])
    c = np.zeros(n)
    pr = np.asarray(retail, np.float64) * dt
    c[ch:ch + T] += pr
    c[dis:dis + T] += -pr + bat.get("OMexpenses", 0.0) / 1000.0 * dt
    c[ec:ec + T] += pr
    if J:
        c[tau:tau + J] = dprice
    c0 = float(pr @ base) + bat.get("fixedOM", 0.0) * bat["Pdis"] + fixed_om
    l, u = np.zeros(n), np.zeros(n)
    u[ch:ch + T], u[dis:dis + T] = bat["Pch"], bat["Pdis"]
    l[ene:ene + T], u[ene:ene + T] = bat["llsoc"] * E, bat["ulsoc"] * E
    l[tau:tau + J], u[tau:tau + J] = -np.inf, np.inf
    u[ec:ec + T] = np.where(pl, ch_max, 0.0)
    l[ee:ee + T], u[ee:ee + T] = -np.inf, np.inf
    return dict(K=sp.csr_matrix(np.array(rows)), q=np.array(q), c=c, c0=c0, l=l, u=u, m_eq=m_eq)


def state_of(plugged, dt, ev_ch):
    """The reference's ev_ene on plugged steps for a charging series ev_ch [T] (zero elsewhere): its rows solved
    forward from every plug-in step."""
    pl = np.asarray(plugged, bool)
    e = np.zeros(len(pl))
    for t in range(1, len(pl)):
        if pl[t] and pl[t - 1]:
            e[t] = e[t - 1] + dt * ev_ch[t - 1]
    return e


def shift_form_accepts(lp):
    """The set-up check of pdhg_band_shift_kernel<768> (csrc/dvh_band_shift.hip, "structure check") on a WindowLP:
    True where the kernel takes the window, False where it hands it on."""
    B, JMAX, SMALL = 768, 4, 4096
    n, m, meq = len(lp.c), len(lp.q), lp.m_eq
    ip, ix, lo, hi = lp.indptr, lp.indices, lp.l, lp.u
    if n > SMALL or m > SMALL or meq < 4 or m < meq or ip[-1] < 1 or ip[1] - ip[0] != 1:
        return False
    c00 = int(ix[ip[0]])
    T = c00 >> 1
    J, D = n - 5 * T, meq - 2 * T - 1
    if c00 < 2 or (c00 & 1) or T > B or J < 0 or J > JMAX or D < 1 or D > T:
        return False
    CPW, CE = 3 * T + J, 4 * T + J
    if not (np.all(lo[3 * T:CPW] == -np.inf) and np.all(hi[3 * T:CPW] == np.inf)):
        return False
    for r in range(1, T + 1):  # the battery's rows
        t = r - 1
        cols = sorted(ix[ip[r]:ip[r + 1]].tolist())
        if cols != sorted([t, T + t, 2 * T + t] + ([2 * T + t + 1] if r < T else [])):
            return False
        if lo[t] != 0.0 or lo[T + t] != 0.0 or lo[CE + t] != 0.0:
            return False
    lrow, srow, dcm = {}, {}, {}
    for i in range(T + 1, meq):  # the load's equality rows
        cols = ix[ip[i]:ip[i + 1]].tolist()
        if not 1 <= len(cols) <= 3:
            return False
        if len(cols) == 1:
            t = cols[0] - CE
            if not 0 <= t < T or t in srow:
                return False
            srow[t] = i
            continue
        tp = [c - CPW for c in cols if CPW <= c < CE]
        if len(tp) != 1:
            return False
        t = tp[0]
        want = [CPW + t, CE + t] + ([CE + t + 1] if len(cols) == 3 and t + 1 < T else [])
        if sorted(cols) != want or t in lrow:
            return False
        lrow[t] = i
    for i in range(meq, m):  # DCM epigraph rows
        cols = ix[ip[i]:ip[i + 1]].tolist()
        if not 3 <= len(cols) <= 4:
            return False
        tc = [c for c in cols if 0 <= c < T]
        td = [c - T for c in cols if T <= c < 2 * T]
        jj = [c for c in cols if 3 * T <= c < CPW]
        tp = [c - CPW for c in cols if CPW <= c < CE]
        if len(tc) != 1 or td != tc or len(jj) != 1 or len(tc) + len(td) + len(jj) + len(tp) != len(cols):
            return False
        if len(tp) > 1 or (tp and tp != tc) or tc[0] in dcm:
            return False
        dcm[tc[0]] = i
    return len(lrow) == T
