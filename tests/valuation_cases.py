"""Shared inputs of the valuation tests (tests/test_valuation_native.py: csrc/dvh_cba.h on the host;
tests/test_gpu_valuation.py: the kernels), and the comparison they apply against the numpy host form."""
import numpy as np

from dervet_hip import valuation as V


def bill_group(T, J, G, pv=False, ice=False, negative=False, da=False, own_orig=True, seed=0):
    """One window group and random feasible dispatch vectors x [G, n] (layout [ch, dis, ene, tau, pv?, elec?, on?]).
    J = 3: mask 0 covers every step, mask 1 every third step (they overlap), mask 2 is one step.  negative: the net
    load is below zero at every step, so the peaks are negative."""
    rng = np.random.default_rng([T, J, G, seed])
    masks = [np.ones(T, bool), np.arange(T) % 3 == 0, np.arange(T) == T - 1][:J]
    rows = [np.nonzero(m)[0] for m in masks]
    dcm_t = np.concatenate(rows).astype(np.int32) if J else np.zeros(0, np.int32)
    dcm_j = np.concatenate([np.full(len(r), j) for j, r in enumerate(rows)]).astype(np.int32) if J else np.zeros(0, np.int32)
    base = rng.uniform(-900.0, -500.0, (G, T)) if negative else rng.uniform(400.0, 900.0, (G, T))
    inp = V.BillInputs(T=T, J=J, dt=0.25 if T % 2 else 1.0, dcm_t=dcm_t, dcm_j=dcm_j, base=base,
                       retail=rng.uniform(0.05, 0.3, (G, T)), da=rng.uniform(0.01, 0.1, (G, T)) if da else None,
                       demand=rng.uniform(5.0, 20.0, (G, J)), om=rng.uniform(0.0, 5.0, G),
                       ice_cost=rng.uniform(0.1, 0.4, G) if ice else None, has_pv=pv,
                       orig=rng.uniform(500.0, 1200.0, (G, T)) if own_orig else None)
    x = rng.uniform(0.0, 100.0, (G, inp.need))
    x[:, 2 * T:3 * T + J] = rng.normal(size=(G, T + J)) * 1e6   # ene / tau: must not matter
    if ice:
        x[:, -T:] = rng.uniform(0.0, 1.0, (G, T))               # on
    return inp, x


def bill_cases():
    """T in {1, 2, 63, 64, 65, 255, 256, 257, 744} x J in {0, 1, 3} x the column blocks, G in {1, 257}; every case has
    one window that is not OPTIMAL when G > 1."""
    out = []
    blocks = [(False, False), (True, False), (False, True), (True, True)]
    for i, T in enumerate((1, 2, 63, 64, 65, 255, 256, 257, 744)):
        for J in (0, 1, 3):
            pv, ice = blocks[(i + J) % 4]
            G = 257 if (T, J) == (65, 3) else (3 if T < 744 else 2)
            if (T, J) == (64, 1):
                G = 1
            inp, x = bill_group(T, J, G, pv=pv, ice=ice, negative=(T, J) in ((63, 3), (257, 1)), da=J != 1,
                                own_orig=J != 0)
            status = np.zeros(G, np.int32)
            if G > 1:
                status[1] = 3
            out.append(dict(id=f"T{T}-J{J}-G{G}{'-pv' if pv else ''}{'-ice' if ice else ''}", inp=inp, x=x, status=status))
    return out


def value_case(S, Y, n_opt=1, per=12, seed=0, n_extra=2, shuffle=False):
    """S scenarios of `per` windows per opt year.  With S > 1: scenario 1 has no IRR (every flow is positive: a negative
    capital cost, no variable or fixed cost), scenario 2 misses its first window (valid = 0 when that empties the opt year: per = 1),
    scenario 3 has a flagged window with NaN dispatch rows, scenario 4 no capital cost.
    shuffle: the bill rows in a random packing order (the CSR map follows; same values)."""
    rng = np.random.default_rng([S, Y, n_opt, seed])
    opt = tuple(sorted(rng.choice(Y, n_opt, replace=False).tolist())) if n_opt > 1 else (min(Y - 1, 1),)
    nb = S * per * n_opt
    bills = np.empty((nb, V.BILL_ROWS))
    bills[:, :5] = rng.uniform(100.0, 3000.0, (nb, 5))
    bills[:, 5:] = bills[:, [V.RETAIL, V.DEMAND, V.DA]] + rng.uniform(50.0, 2500.0, (nb, 3))
    bad = np.zeros(nb, np.int32)
    idx = np.arange(nb)
    year = np.repeat(np.tile(np.asarray(opt), S), per)
    cnt = np.full(S, per * n_opt)
    capex = rng.uniform(0.5, 8.0, S) * per * 4000.0
    if S > 1:
        capex[1] = -1e9
        bills[per * n_opt:2 * per * n_opt, [V.VAR_OM, V.FUEL]] = 0.0
        capex[4 % S] = 0.0
        k = 3 * per * n_opt + 1
        bad[k] = 1
        bills[k, :5] = np.nan
        drop = 2 * per * n_opt          # scenario 2 loses its first window
        idx, year = np.delete(idx, drop), np.delete(year, drop)
        cnt[2] -= 1
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    if shuffle:
        perm = np.random.default_rng(nb).permutation(nb)   # row r of the table moves to perm[r]
        shuffled, sbad = np.empty_like(bills), np.empty_like(bad)
        shuffled[perm], sbad[perm] = bills, bad
        bills, bad, idx = shuffled, sbad, perm[idx]
    fixed_om = rng.uniform(0.0, 2000.0, S)
    fixed_om[1 % S] = 0.0
    fin = V.Financials(years=Y, opt_years=opt, rate=0.06, growth=[2.2, 2.2, 1.0, 3.0, -0.5], capex=capex,
                       fixed_om=fixed_om, extra=rng.uniform(0.0, 400.0, (n_extra, Y + 1)))
    return dict(id=f"S{S}-Y{Y}-opt{n_opt}-per{per}", bills=bills, bad=bad, ptr=ptr, idx=idx.astype(np.int32),
                year=year.astype(np.int32), fin=fin)


def value_cases():
    out = [value_case(S, Y) for S in (1, 65) for Y in (1, 21, 64)]
    out.append(value_case(65, 21, n_opt=2, seed=1))
    out.append(value_case(65, 64, n_opt=3, per=1, seed=2))   # a dropped window empties an opt year: valid = 0
    return out


def assert_case_is_what_it_says(want):
    """On the host form's result of a value_case: the scenarios built to be special are."""
    assert want.valid[0] == 1 and np.isfinite(want.npv[0])
    if len(want.valid) > 1:
        assert np.isnan(want.irr[1]) and np.isfinite(want.npv[1])
        assert want.valid[3] == 0 and np.isnan(want.npv[3])
        assert np.isfinite(want.irr).sum() > len(want.valid) // 2


def assert_valuations_agree(got, want, rtol=1e-12, irr_atol=1e-10):
    """got against the numpy host form: the flag and the NaN pattern exactly, sums within rtol, IRR within irr_atol."""
    assert np.array_equal(np.asarray(got.valid), np.asarray(want.valid))
    gv, wv = np.asarray(got.values), np.asarray(want.values)
    assert np.array_equal(np.isnan(gv), np.isnan(wv))
    np.testing.assert_allclose(gv[:, :6], wv[:, :6], rtol=rtol, atol=0.0)
    np.testing.assert_allclose(gv[:, 6], wv[:, 6], rtol=0.0, atol=irr_atol)
    if got.proforma is not None and want.proforma is not None:
        assert np.array_equal(np.isnan(got.proforma), np.isnan(want.proforma))
        np.testing.assert_allclose(got.proforma, want.proforma, rtol=rtol, atol=0.0)
