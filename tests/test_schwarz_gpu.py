"""GPU tests of the Schwarz factors and of screened builds at thresholds where screening bites, against the CPU oracle.

Every direct Fock build and two-electron gradient runs on work lists screened with factors the GPU computed itself, in a mode of the
class kernels nothing else uses (`schwarz_out`: unsplit slots of the column kernels, one-ket bundles of the bra-major kernels); the
largest factor also sets the scale of the fixed-point accumulation.  On the shipped, compact molecules the default threshold drops only
what is below the parity bar anyway, so a wrongly screened build looks like a correctly screened one.  spread() (synthetic_systems.py:
five centres over 19 bohr, n = 37, 13 shells, 91 shell pairs of which 12 fall under the primitive cut-off and are not stored, 4186
unique quartets) has factors from 7e-42 to 1.37.  Working thresholds - the geometric middle of the widest gap between consecutive
sorted products Q_P Q_Q within a decade of the nominal value, recomputed here from the reference factors - on the CPU, RHF,
D = rand_sym(37, 51), max|G_ref| = 0.53:

    nominal tau   working tau   gap ratio   share dropped   max|G_pred - G_ref|
    1e-12         1.5032e-13    1.198       47.1 %          2.7e-14
    1e-9          3.6534e-9     1.167       60.1 %          7.0e-10
    1e-6          1.5761e-7     1.097       64.0 %          6.8e-8
    1e-3          6.7564e-3     1.129       88.0 %          1.7e-3
    (tetra-pure-2, n = 64: 3.7322e-4, 1.026, 11.2 %, 3.0e-4 - its 9316 products crowd into five decades: no threshold there has both a
    5 % gap and a 30 % share, so that case asserts a 1 % gap and a 10 % share; see test_screened_builds_on_tetra)

References: Q_ref[P] = sqrt(max over the diagonal of the (P|P) block) of the oracle's dense tensor; the kept set and the mask
mask[i, j, k, l] = Qf[i, j] Qf[k, l] >= tau follow from Q_ref alone (schwarz_reference.py).

The bar on the factors (2a) is relative, SCHWARZ_BAR = 1.04e-12: 100 times the largest relative disagreement between the oracle's
factors and two independent columns (numpy/scipy eri_block, and mpmath at 50 digits for the ss pairs), 1.04e-14, measured by
test_schwarz_host.py on the CPU; floored at 1e-13.  Builds are compared at TOL_INT = 1e-10 times max(1, |G_pred|max), gradient terms
at 1e-9 times max(1, |fd|), as everywhere in the suite.

A pair the library does not store has every primitive pair's Hermite block below QC_PRIM_CUTOFF = 1e-17 (qc_system.cpp; the block
carries the coefficients, the Gaussian-product factor and sqrt(2) pi^(5/4) / p of the prefactor).  (ab|ab) is then a sum over K^2
primitive quartets, K = nprim_a nprim_b, of H^2 products E_ab E_ab' R / sqrt(p + q), H = (L+1)(L+2)(L+3)/6 Hermite components,
L = l_a + l_b, each below 1e-34 times the O(10) the comment there gives for the remaining factor: Q_ref <= 1e-17 K H sqrt(10), which is
at most 1e-17 * 169 * 84 * 3.2 = 4.5e-13 for anything this library accepts, and far below the 1e-8 that would matter to a 1e-10 bar.

Measured on the MI355X (the tests print these):
    2a  largest |Q - Q_ref| / Q_ref: spread 1.47e-14, deep 7.96e-15, tetra-pure-2 1.21e-15, water/cc-pVTZ 3.26e-15 (spread: 9.58e-10
        while the primitive cut-off was absolute only, see test_schwarz_factors_match_reference)
    2b  kept / predicted quartets 2215, 501, 1671, 3160, 1505 in the order visited: equal sets each time
    2c  largest |G - G_pred| / max(1, |G_pred|max): spread 2.1e-15 (all five thresholds, RHF and UHF), tetra-pure-2 6.7e-15
    2e  largest |analytic - stencil| / max(1, |stencil|): 3.3e-13 near 1e-6, 3.7e-13 near 1e-3 (the mask moves the stencil by 1.3e-3)
    2f  2^30: bit for bit; 2^-30: 9.6e-25 against a bar of 5.3e-14; sum|D| = 1e6: 3.8e-9 against 6.8e-9
    2g  max |ERI - oracle| 1.6e-15 at either threshold, bit for bit equal (before the fix of the tensor launch's LDS sizes: 1.3e+296 near 1e-3)"""
import numpy as np
import pytest

import schwarz_reference as sr
import synthetic_systems as syn
from conftest import load_system
from test_gpu_parity import TOL_INT
from test_schwarz_host import SCHWARZ_BAR

pytestmark = pytest.mark.gpu

QC_PRIM_CUTOFF = 1e-17          # qc_internal.h
SYSTEMS = ["spread", "deep", "tetra-pure-2", "water/cc-pVTZ"]
VISITS = (1e-12, 1e-3, 1e-9, 0.0, 1e-6)          # nominal thresholds in the order one handle sees them: up, down, off, on again


@pytest.fixture(scope="module")
def refs():
    """name -> (MolecularSystem, Oracle, oracle tensor, Q_ref by shell pair, Q_ref by function pair), built on first use, unchanged"""
    from oracle.oracle import Oracle
    cache = {}

    def get(name):
        if name not in cache:
            m = load_system(*name.split("/")) if "/" in name else syn.BUILDERS[name]()[0]
            o = Oracle(m)
            I = syn.oracle_tensor(o)
            I.setflags(write=False)
            Q = sr.pair_factors(o, I)
            Qf = sr.function_factors(o, Q)
            Qf.setflags(write=False)
            cache[name] = (m, o, I, Q, Qf)
        return cache[name]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def spread_taus(refs):
    """nominal -> working threshold of spread, with the preconditions the tests rest on asserted on the reference alone"""
    Q = refs("spread")[3]
    prod = sr.quartet_products(Q)[0]
    taus = {0.0: 0.0}
    for nominal in sr.NOMINAL_TAUS:
        tau, ratio = sr.working_tau(prod, nominal)
        share = float(np.mean(prod < tau))
        assert ratio >= 1.05 and 0.30 <= share <= 0.95, (nominal, tau, ratio, share)
        taus[nominal] = tau
    return taus


def _stored(s):
    ab, Qg = s.schwarz_factors()
    return [tuple(p) for p in ab.tolist()], Qg


def _kept(s):
    return sorted(sr.canonical(*t) for t in s.plan_shard_quartets(0, 1).tolist())


def _cutoff_bound(o, pair):
    """QC_PRIM_CUTOFF K H sqrt(10) of a shell pair (module docstring): the most Q_ref can be for a pair that is not stored"""
    tab = o.shell_table()
    K, L = tab[pair[0]][3] * tab[pair[1]][3], tab[pair[0]][2] + tab[pair[1]][2]
    return QC_PRIM_CUTOFF * K * ((L + 1) * (L + 2) * (L + 3) // 6) * np.sqrt(10.0)


@pytest.fixture(scope="module")
def factors(refs):
    """name -> (stored pairs, the GPU's factors) of a fresh handle, read once"""
    import qchem_rs_amd as q
    cache = {}

    def get(name):
        if name not in cache:
            s = q.System(refs(name)[0])
            cache[name] = _stored(s)
            s.close()
        return cache[name]
    return get


# ---- 2a
@pytest.mark.parametrize("name", SYSTEMS)
def test_schwarz_factors_match_reference(name, refs, factors):
    """The pairs returned are the shell pairs A >= B in the library's order minus those it did not store; a pair that is not stored
    has Q_ref <= QC_PRIM_CUTOFF K H sqrt(10) <= 1e-8 (module docstring); every factor returned is Q_ref of ITS pair,
    |Q - Q_ref| <= SCHWARZ_BAR Q_ref with Q_ref from the oracle's full tensor; and max Q^2 - the bound on every integral that the
    fixed-point scale rests on - is the largest |(ij|kl)| of the reference.  spread: factors down to 3e-17 stored, twelve pairs not
    stored, so the library's pair index is not the triangular index; deep: 169-primitive pairs, unpacked one-ket bundles in the pass;
    tetra-pure-2: every class, contracted; water/cc-pVTZ: f in a real basis.

    spread missed the bar while the primitive cut-off was absolute only: 11 of its 79 stored pairs, the worst the pair of shells
    (6, 2) - contracted s shells 9.5 bohr apart - with Q = 7.940174023295849e-10 against Q_ref = 7.940174030899261e-10, 9.58e-10
    relative.  Six of that pair's nine primitive pairs were below 1e-17 and not stored; the closed form of tools/gen_golden.py over
    the three stored ones alone gives 7.940174023295841e-10, the GPU's value: the kernels were right, the stored pair was short.  A weak
    pair now keeps its primitive pairs down to 1e-13 of its largest block (QC_PRIM_REL, qc_system.cpp): 1.47e-14 at the worst pair."""
    m, o, I, Q, _ = refs(name)
    pairs, Qg = factors(name)
    every = sr.pair_list(Q)
    assert len(set(pairs)) == len(pairs) and set(pairs) <= set(every)
    assert pairs == [p for p in every if p in set(pairs)]                    # a ascending, b <= a ascending
    missing = [p for p in every if p not in set(pairs)]
    for p in missing:
        assert Q[p] <= _cutoff_bound(o, p) <= 1e-8, (p, Q[p], _cutoff_bound(o, p))
    if name == "spread":
        assert missing and min(Q[p] for p in pairs) < 1e-15
    rel = np.array([abs(g - Q[p]) / Q[p] for p, g in zip(pairs, Qg)])
    worst = int(np.argmax(rel))
    print("%s: %d of %d pairs stored, Q from %.2e to %.2e; largest |Q - Q_ref| / Q_ref = %.2e at pair %s (bar %.2e)"
          % (name, len(pairs), len(Q), Qg.min(), Qg.max(), rel[worst], pairs[worst], SCHWARZ_BAR))
    over = [(p, float(r)) for p, r in zip(pairs, rel) if r > SCHWARZ_BAR]
    assert not over, (len(over), "worst", pairs[worst], Qg[worst], Q[pairs[worst]], over[:8])
    imax_ref = float(np.abs(I).max())
    assert abs(Qg.max() ** 2 - imax_ref) <= SCHWARZ_BAR * imax_ref, (Qg.max() ** 2, imax_ref)


# ---- 2b
def test_screening_decisions_follow_the_reference_factors(refs, spread_taus):
    """The kept quartets at four working thresholds and at 0, visited on ONE handle in the order 1e-12, 1e-3, 1e-9, 0, 1e-6 (a list left
    over from the threshold before would show), are exactly the set the rule Q_P Q_Q >= tau predicts from Q_ref - the gaps make that
    insensitive to rounding -, and the counters add up: enumerated = kept + screened out + quartets with a pair that is not stored.
    Last, tau exactly ON a product of the library's own factors: that quartet stays (the rule is >=, not >)."""
    import qchem_rs_amd as q
    m, o, I, Q, _ = refs("spread")
    s = q.System(m)
    pairs, Qg = _stored(s)
    ws = s.work_stats()
    assert ws.schwarz_tau == 1e-12 and ws.quartets_enumerated == s.n_quartets() == 4186
    n_unstored = 4186 - len(pairs) * (len(pairs) + 1) // 2
    assert n_unstored > 0
    sizes = []
    for nominal in VISITS:
        tau = spread_taus[nominal]
        s.set_schwarz(tau)
        kept, want = _kept(s), sr.predicted(Q, tau, pairs)
        ws = s.work_stats()
        sizes.append(len(kept))
        print("tau %.4e (nominal %.0e): %d quartets kept, %d predicted, %d screened out" % (tau, nominal, len(kept), len(want), ws.quartets_screened_out))
        assert kept == want, (nominal, len(kept), len(want), sorted(set(kept) ^ set(want))[:5])
        assert ws.schwarz_tau == tau and ws.quartets == len(kept)
        assert ws.quartets_enumerated - ws.quartets - ws.quartets_screened_out == n_unstored
    assert len(set(sizes)) == len(sizes) and sizes[3] == len(pairs) * (len(pairs) + 1) // 2
    # tau on a product: the first product above the working threshold near 1e-6, from the library's own two factors (one
    # multiplication, commutative: the very double the rule compares with); the next product up is a reference-sized step away
    prod, P, K, pl = sr.quartet_products(Q, pairs)
    order = np.argsort(prod)
    k = int(np.searchsorted(prod[order], spread_taus[1e-6]))
    assert prod[order[k + 1]] / prod[order[k]] > 1 + 1e-6 and prod[order[k]] / prod[order[k - 1]] >= 1.05
    qg = dict(zip(pairs, Qg))
    tau_on = qg[pl[P[order[k]]]] * qg[pl[K[order[k]]]]
    assert abs(tau_on - prod[order[k]]) <= 1e-6 * tau_on          # (the same product: its neighbours are 0.4 % and 9 % away)
    s.set_schwarz(tau_on)
    assert _kept(s) == sr.predicted(Q, spread_taus[1e-6], pairs)
    s.close()


# ---- 2c
def _check_builds(s, o, I, Qf, tau, what, tol_factor_needed):
    """fock_rhf for two seeds and fock_uhf (Da != Db) at threshold tau against the dense contraction of the masked tensor; returns the
    largest error over the scale.  tol_factor_needed: the mask must move G by at least that many tolerances (0: not asserted)"""
    Im = I * sr.function_mask(Qf, tau)
    worst = 0.0
    for seed in (51, 52):
        D = syn.rand_sym(s.n, seed)
        G_pred = o.g_rhf(D, Im)
        tol = TOL_INT * max(1.0, np.abs(G_pred).max())
        moved = float(np.abs(G_pred - o.g_rhf(D, I)).max())
        assert moved >= tol_factor_needed * tol, (what, seed, moved, tol)
        G = s.fock_rhf(D)
        err = float(np.abs(G - G_pred).max())
        worst = max(worst, err / (tol / TOL_INT))
        assert err <= tol, (what, "rhf", seed, err, tol, moved)
        assert np.array_equal(G, G.T), (what, "rhf", seed)
    Da, Db = syn.rand_sym(s.n, 53), syn.rand_sym(s.n, 54)
    Ga, Gb = s.fock_uhf(Da, Db)
    for X, R, spin in ((Ga, o.g_uhf(Da, Db, Im), "alpha"), (Gb, o.g_uhf(Db, Da, Im), "beta")):
        tol = TOL_INT * max(1.0, np.abs(R).max())
        err = float(np.abs(X - R).max())
        worst = max(worst, err / (tol / TOL_INT))
        assert err <= tol, (what, "uhf", spin, err, tol)
        assert np.array_equal(X, X.T), (what, "uhf", spin)
    print("%s, tau %.4e: max |G - G_pred| / scale = %.3e (tolerance %.0e)" % (what, tau, worst, TOL_INT))
    return worst


def test_screened_builds_equal_the_masked_contraction(refs, spread_taus):
    """spread at the four working thresholds and at 0, one handle, same order of visits: RHF for two seeds and UHF with two different
    densities equal the contraction of I_ref * mask; at the two largest thresholds the mask moves G by at least 100 tolerances (1.7e-3
    and 6.8e-8 against 1e-10), so a build that screened other quartets than the rule says could not pass.  At 6.76e-3 the class
    LAB = 5, LCD = 5 keeps nothing, the (ss|ss) class keeps 46 quartets - less than one 64-ket bundle."""
    import qchem_rs_amd as q
    m, o, I, Q, Qf = refs("spread")
    s = q.System(m)
    for nominal in VISITS:
        tau = spread_taus[nominal]
        s.set_schwarz(tau)
        _check_builds(s, o, I, Qf, tau, "spread", 100 if nominal in (1e-6, 1e-3) else 0)
    s.close()


def test_screened_builds_on_tetra(refs):
    """tetra-pure-2 (n = 64: the replica count of n <= 64, every class kernel with four distinct centres, contracted shells) at the
    working threshold near 1e-3 by the same gap rule.  Its factors span 0.003 .. 1.3 only and its 9316 products lie so densely that no
    threshold has both a 5 % gap and a 30 % dropped share (the widest gap within a decade of 1e-3 is 2.6 %, 11 % dropped; the first 5 %
    gap above it drops 98.5 %).  Asserted on the reference instead: a gap of at least 1 % - ten orders above the 1e-12 the factors are
    pinned to by test_schwarz_factors_match_reference, so no decision depends on rounding -, at least 10 % dropped, and G moved by at
    least 100 tolerances (3e-4 against 1e-10)."""
    import qchem_rs_amd as q
    m, o, I, Q, Qf = refs("tetra-pure-2")
    prod = sr.quartet_products(Q)[0]
    tau, ratio = sr.working_tau(prod, 1e-3)
    share = float(np.mean(prod < tau))
    print("tetra-pure-2: working tau %.4e, gap ratio %.4f, %.1f %% dropped" % (tau, ratio, 100 * share))
    assert ratio >= 1.01 and 0.10 <= share <= 0.95
    s = q.System(m)
    pairs, _ = _stored(s)
    assert len(pairs) == len(Q)
    s.set_schwarz(tau)
    assert _kept(s) == sr.predicted(Q, tau, pairs)
    _check_builds(s, o, I, Qf, tau, "tetra-pure-2", 100)
    s.close()


def test_sharded_screened_builds_sum_to_the_full_one(refs, spread_taus):
    """spread at the working threshold near 1e-3: the partial matrices of three shards sum to the screened G (1e-11 |G|max, as in
    test_sharded_fock_sums_to_full) - classes with fewer kept quartets than ranks, one of them empty - and that G is the masked one."""
    import qchem_rs_amd as q
    m, o, I, Q, Qf = refs("spread")
    tau = spread_taus[1e-3]
    s = q.System(m)
    s.set_schwarz(tau)
    D = syn.rand_sym(s.n, 51)
    G_full = s.fock_rhf(D)
    G_pred = o.g_rhf(D, I * sr.function_mask(Qf, tau))
    assert np.abs(G_full - G_pred).max() <= TOL_INT * max(1.0, np.abs(G_pred).max())
    acc, nq = np.zeros_like(G_full), 0
    for r in range(3):
        s.set_shard(r, 3)
        nq += s.work_stats().quartets
        acc += s.fock_rhf(D)
    s.set_shard(0, 1)
    assert nq == s.work_stats().quartets == len(sr.predicted(Q, tau, _stored(s)[0]))
    assert np.abs(acc - G_full).max() <= 1e-11 * np.abs(G_full).max()
    assert np.array_equal(s.fock_rhf(D), G_full)
    s.close()


# ---- 2d
def test_everything_screened_out(refs):
    """tau = 10 times the largest product (finite): no quartet left, no launch; fock_rhf and fock_uhf return exact zeros with status
    OK and the two-electron gradient term is exactly zero while the other terms are not; NaN and negative thresholds are refused and
    change nothing; back at 0 the handle builds the unscreened G."""
    import qchem_rs_amd as q
    m, o, I, Q, Qf = refs("spread")
    s = q.System(m)
    tau = 10.0 * max(Q.values()) ** 2
    assert np.isfinite(tau)
    D, W = syn.rand_sym(s.n, 51), syn.rand_sym(s.n, 12)
    G_before = s.fock_rhf(D)
    s.set_schwarz(tau)
    ws = s.work_stats()
    assert ws.quartets == 0 and ws.nclasses == 0 and len(s.plan_shard_quartets(0, 1)) == 0
    assert ws.quartets_screened_out == len(_stored(s)[0]) * (len(_stored(s)[0]) + 1) // 2
    G = s.fock_rhf(D)
    assert G.shape == (s.n, s.n) and not G.any()
    Ga, Gb = s.fock_uhf(D, 0.5 * D)
    assert not Ga.any() and not Gb.any()
    vnn, core, ovl, two = s.gradient(D, W)
    assert not two.any() and np.abs(core).max() > 1e-3 and np.abs(ovl).max() > 1e-3
    two_u = s.gradient(D, W, Db=0.5 * D)[3]
    assert not two_u.any()
    for bad in (float("nan"), -1.0):
        with pytest.raises(q.hf.QcError, match="invalid argument"):
            s.set_schwarz(bad)
        assert s.work_stats().schwarz_tau == tau and s.work_stats().quartets == 0
    s.set_schwarz(1e-12)
    assert np.array_equal(s.fock_rhf(D), G_before)
    s.set_schwarz(0.0)
    G0 = s.fock_rhf(D)
    G_ref = o.g_rhf(D, I)
    assert np.abs(G0 - G_ref).max() <= TOL_INT * max(1.0, np.abs(G_ref).max())
    s.close()


# ---- 2e
GRAD_COORDS = [(0, 0), (4, 1), (2, 2)]          # an atom of a kept near pair, the far atom, the f centre - one axis each


@pytest.mark.parametrize("nominal", [1e-6, 1e-3])
def test_gradient_under_screening_is_the_derivative_over_the_kept_quartets(nominal, refs, spread_taus):
    """The two-electron term of qc_gradient - whose task list restates the screening rule - at fixed random densities, RHF and UHF,
    against the five-point stencil of the oracle's energy over the kept integrals: the mask is fixed at the central geometry and
    applied to the tensor of every displaced geometry.  Near 1e-3 the unmasked stencil differs from the masked one by more than 1e-6
    (a thousand tolerances) at one coordinate at least: a gradient that screened nothing, or other quartets, fails."""
    import qchem_rs_amd as q
    m, o, I, Q, Qf = refs("spread")
    assert [int(m.shell_L[i]) for i in range(m.n_shells) if m.shell_atom[i] == 2] == [0, 1, 3]
    tau = spread_taus[nominal]
    mask = sr.function_mask(Qf, tau)
    s = q.System(m)
    s.set_schwarz(tau)
    n = s.n
    P, W = syn.rand_sym(n, 11), syn.rand_sym(n, 12)
    Da, Db, Wu = syn.rand_sym(n, 13), syn.rand_sym(n, 14), syn.rand_sym(n, 15)
    two_r = s.gradient(P, W)[3]
    two_u = s.gradient(Da, Wu, Db=Db)[3]
    worst, moved = 0.0, 0.0
    for c in GRAD_COORDS:
        for an, dens in ((two_r[c], (P, 0.5 * P, 0.5 * P, W)), (two_u[c], (Da + Db, Da, Db, Wu))):
            fd = syn.fd_terms(m, c, *dens, mask=mask)[3]
            if nominal == 1e-3:
                moved = max(moved, abs(fd - syn.fd_terms(m, c, *dens)[3]))
            worst = max(worst, abs(an - fd) / max(1.0, abs(fd)))
            assert abs(an - fd) <= 1e-9 * max(1.0, abs(fd)), (c, an, fd)
    print("spread, tau %.4e: two-electron gradient against the masked stencil, max error / scale %.3e (tolerance 1e-9)" % (tau, worst))
    if nominal == 1e-3:
        print("the mask moves the stencil by up to %.3e" % moved)
        assert moved > 1e-6, moved
    s.close()


# ---- 2f
def test_fixed_point_scale_follows_the_density(refs):
    """The unit of the fixed-point accumulation is 2^-S, S = min(QC_FX_MAXBITS = 52, 60 - ceil(log2(4 imax sum|D|)))
    (qc_fx_scale_kernel): for D = rand_sym(37, 51), 4 imax sum|D| is about 830 and S = 50.  Scaling D by 2^30 moves S by exactly 30
    bits (20: not clamped), every contribution is the same integer, so fock_rhf(s D) == s fock_rhf(D) bit for bit.  Scaling by 2^-30
    asks for S = 80 and is clamped to 52 - the small-density side is the one that clamps: the unit no longer follows the density, the
    roundings differ, and the comparison is |fock_rhf(s D) - s fock_rhf(D)| <= 1e-13 |G|max, G = fock_rhf(D) (rounding to a fixed unit
    is an absolute error: it does not shrink with s).  A density with sum|D| = 1e6 (S = 37)
    against the dense contraction at 1e-12 |G_ref|max: a factor too small by 2^2 or more in imax would let the 64-bit sums wrap."""
    import qchem_rs_amd as q
    m, o, I, Q, Qf = refs("spread")
    s = q.System(m)
    D = syn.rand_sym(s.n, 51)
    bound = 4.0 * max(Q.values()) ** 2 * np.abs(D).sum()
    S0 = 60 - int(np.frexp(bound)[1])
    assert S0 <= 52 and S0 - 30 >= -900 and S0 + 30 > 52          # which side clamps, from the reference
    G = s.fock_rhf(D)
    up = 2.0 ** 30
    assert np.array_equal(s.fock_rhf(up * D), up * G)
    down = 2.0 ** -30
    err = float(np.abs(s.fock_rhf(down * D) - down * G).max())
    print("fock_rhf(2^-30 D) against 2^-30 fock_rhf(D): %.3e (bar %.3e)" % (err, 1e-13 * np.abs(G).max()))
    assert err <= 1e-13 * np.abs(G).max()
    big = D * (1e6 / np.abs(D).sum())
    G_ref = o.g_rhf(big, I)
    err = float(np.abs(s.fock_rhf(big) - G_ref).max())
    print("sum|D| = 1e6: max |G - G_ref| = %.3e, |G_ref|max = %.3e" % (err, np.abs(G_ref).max()))
    assert err <= 1e-12 * np.abs(G_ref).max()
    s.close()


# ---- 2g
def test_the_tensor_is_not_screened(refs, spread_taus):
    """qc_eri_full runs over every class's whole task list, not the screened shard: at the working threshold near 1e-3, which drops
    88 % of the quartets from the builds and empties a class, the tensor matches the oracle and is bit for bit the tensor at 0.
    (It was not: the tensor launch of a column class took its LDS size per lane group from the screened shard - zero words for an
    emptied class - so lane groups overlapped: max |ERI - oracle| = 1.3e+296 near 1e-3 on the MI355X before the fix, 1.6e-15 after.)"""
    import qchem_rs_amd as q
    m, o, I, Q, Qf = refs("spread")
    s = q.System(m)
    _stored(s)                                   # (the device pass has run: from here on the work lists are screened)
    s.set_schwarz(spread_taus[1e-3])
    assert s.work_stats().quartets < 0.2 * 4186
    I_screened = s.eri()
    s.set_schwarz(0.0)
    I_open = s.eri()
    print("max |ERI - oracle|: %.3e at tau %.4e, %.3e at 0" % (np.abs(I_screened - I).max(), spread_taus[1e-3], np.abs(I_open - I).max()))
    assert np.abs(I_open - I).max() <= TOL_INT
    assert np.abs(I_screened - I).max() <= TOL_INT
    assert np.array_equal(I_open, I_screened)
    s.close()
