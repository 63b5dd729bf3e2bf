"""A controllable (load-shifting) load on a plain battery window, restated densely and independently of
dervet_hip.lp.builder from dervet MicrogridDER/LoadControllable.py:233-249, for tests/test_ctrl_load_builder.py and
tests/test_gpu_load_shift.py; and the windows both share (tests/test_gpu_interconnect.py's battery and series).

  x = [ch(T), dis(T), ene(T), tau(J), pw(T), el(T)]
  battery        ene_0 = target; ene_{t+1} = (1 - dt sdr) ene_t + dt eta ch_t - dt dis_t; back to target after T - 1
  load bounds    -P <= pw <= P (:234-235), 0 <= el <= E_L = P x duration (:236-237)
  per day [d0, d1) (:242-249)
                 el_d0 = E_L                            (:247)
                 el_t + dt pw_t - el_{t+1} = 0          (:245)
                 el_{d1-1} + dt pw_{d1-1} = E_L         (:249)
  net load       load_t + ch_t - dis_t + pw_t (get_charge, :120-133): the DCM epigraph tau_j >= net_t on its steps,
                 the retail energy charge price_t dt net_t
"""
import numpy as np
import scipy.sparse as sp

from dervet_hip.lp import builder

BAT = dict(E=2000.0, Pch=500.0, Pdis=500.0, rte=0.9, sdr=0.0, soc_target=0.5, ulsoc=1.0, llsoc=0.1, fixedOM=1.0,
           OMexpenses=0.0, hp=0.0)
P, DH = 150.0, 4.0
every24 = lambda T: list(range(0, T, 24))  # noqa: E731
# (T, J, day_starts): the smallest recurrence; a one-step day first; a day break at the wave boundary with a one-step
# last day; uneven days across a wave boundary; idle lanes past T; the full block
SHAPES = [(2, 0, [0]), (2, 1, [0]), (3, 1, [0, 1]), (5, 1, [0, 2]), (48, 1, [0, 24]), (64, 1, [0, 63]),
          (65, 4, [0, 17, 41]), (129, 1, every24(129)), (744, 4, every24(744)), (768, 1, every24(768))]


def series(T, J, G=2, seed=None):
    """Load, retail price, demand masks and prices as tests/test_gpu_interconnect.py draws them."""
    rng = np.random.default_rng(1000 * T + 10 * J if seed is None else seed)
    t = np.arange(T)
    load = rng.uniform(400.0, 700.0, (G, T))
    retail = rng.uniform(0.05, 0.15, (G, T))
    masks = np.array([t % (J + 1) == j for j in range(J)], bool).reshape(J, T)
    dprice = rng.uniform(8.0, 20.0, (G, J)) if J else None
    return load, retail, masks if J else None, dprice


def group(T, J, day_starts, G=2, seed=None, rated_power=P, duration=DH):
    load, retail, masks, dprice = series(T, J, G, seed)
    cl = None if rated_power is None else dict(rated_power=rated_power, duration=duration, day_starts=day_starts)
    return builder.battery_group(T, 1.0, load, BAT, retail_price=retail, demand_masks=masks, demand_prices=dprice,
                                 ctrl_load=cl)


def dense(T, dt, load, bat, retail, masks, dprice, rated_power, duration, day_starts):
    """One window (load, retail [T]; dprice [J]) as an oracle dict: K (csr), q, c, c0, l, u, m_eq."""
    masks = np.zeros((0, T), bool) if masks is None else np.asarray(masks, bool)
    J = len(masks)
    n = 5 * T + J
    ch, dis, ene, tau, pw, el = 0, T, 2 * T, 3 * T, 3 * T + J, 4 * T + J
    E, eta, sdr = bat["E"], bat["rte"], bat["sdr"] / 100.0
    target, EL = bat["soc_target"] * E, rated_power * duration
    rows, q = [], []

    def row(entries, rhs):
        r = np.zeros(n)
        for j, v in entries:
            r[j] += v
        rows.append(r)
        q.append(rhs)

    row([(ene, 1.0)], target)
    for t in range(T - 1):
        row([(ene + t + 1, 1.0), (ene + t, -(1.0 - dt * sdr)), (ch + t, -dt * eta), (dis + t, dt)], 0.0)
    k = T - 1
    row([(ene + k, 1.0 - dt * sdr), (ch + k, dt * eta), (dis + k, -dt)], target)
    bounds = list(day_starts) + [T]
    for d0, d1 in zip(bounds[:-1], bounds[1:]):
        row([(el + d0, 1.0)], EL)
        for t in range(d0, d1 - 1):
            row([(el + t, 1.0), (pw + t, dt), (el + t + 1, -1.0)], 0.0)
        row([(el + d1 - 1, 1.0), (pw + d1 - 1, dt)], EL)
    m_eq = len(rows)
    base = np.asarray(load, np.float64) + bat.get("hp", 0.0)
    for j in range(J):
        for t in np.nonzero(masks[j])[0]:  # tau_j >= base + ch - dis + pw
            row([(tau + j, 1.0), (ch + t, -1.0), (dis + t, 1.0), (pw + t, -1.0)], base[t])
    c = np.zeros(n)
    pr = np.asarray(retail, np.float64) * dt
    c[ch:ch + T] += pr
    c[dis:dis + T] += -pr + bat.get("OMexpenses", 0.0) / 1000.0 * dt
    c[pw:pw + T] += pr
    if J:
        c[tau:tau + J] = dprice
    c0 = float(pr @ base) + bat.get("fixedOM", 0.0) * bat["Pdis"]
    l, u = np.zeros(n), np.zeros(n)
    u[ch:ch + T], u[dis:dis + T] = bat["Pch"], bat["Pdis"]
    l[ene:ene + T], u[ene:ene + T] = bat["llsoc"] * E, bat["ulsoc"] * E
    l[tau:tau + J], u[tau:tau + J] = -np.inf, np.inf
    l[pw:pw + T], u[pw:pw + T] = -rated_power, rated_power
    u[el:el + T] = EL
    return dict(K=sp.csr_matrix(np.array(rows)), q=np.array(q), c=c, c0=c0, l=l, u=u, m_eq=m_eq)
