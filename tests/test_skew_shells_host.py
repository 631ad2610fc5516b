"""CPU tests of the systems in general position (tests/synthetic_systems.py): the oracle pinned by the independent implementation
on four-centre quartets up to (ff|ff) and on f quartets beyond the tabulated Boys range (tests/golden/skew_quartets_golden.json,
written by tools/gen_golden.py), and the host-only model of the library on every builder."""
import json
import os

import numpy as np
import pytest

import synthetic_systems as syn
from conftest import ROOT
from synthetic_systems import BOYS_SERIES_SWITCH, BOYS_XMAX, BUILDERS, SIZES, T_HIGH, T_LOW


@pytest.fixture(scope="module")
def skew_golden():
    with open(os.path.join(ROOT, "tests", "golden", "skew_quartets_golden.json")) as f:
        return json.load(f)


def _check_eri_blocks(o, g):
    for blk in g["eri_blocks"]:
        v = o.eri_shell_quartet(*blk["shells"])
        assert list(v.shape) == blk["shape"], blk["L"]
        v = v.reshape(-1)
        ref = np.array(blk["values"])
        assert len(ref) == len(v[::blk["stride"]]) and np.abs(ref).max() > 1e-6, blk["L"]
        assert np.abs(v[::blk["stride"]] - ref).max() < 1e-13, blk["L"]
        # the whole block under seeded +-1 signs: an error pattern e with |e|_max < 1e-13 moves such a sum by |e|_2 < 1e-13 sqrt(N)
        for k, ref_sum in enumerate(blk["signed_sums"]):
            assert abs(np.dot(syn.skew_signs(v.size, k), v) - ref_sum) < 1e-13 * np.sqrt(v.size), (blk["L"], k)


@pytest.mark.parametrize("key", ["tetra-pure", "tetra-cart"])
def test_oracle_four_centre_blocks_match_independent_implementation(skew_golden, key):
    """(ff|ff), (fd|ff), (fp|df), (dd|dd), (fs|ps), (pp|pp) with every shell on a centre of its own and no vanishing component of
    P - Q, pure and Cartesian, and the S / T / V blocks of f.f, f.d and d.p pairs on distinct atoms; tolerances of
    test_oracle_known_answers.py."""
    from oracle.oracle import Oracle
    g = skew_golden[key]
    o = Oracle(syn.tetra(key == "tetra-pure", 1)[0])
    assert o.n == g["n"]
    assert sorted(tuple(b["L"]) for b in g["eri_blocks"]) == sorted([(3, 3, 3, 3), (3, 2, 3, 3), (3, 1, 2, 3), (2, 2, 2, 2), (3, 0, 1, 0), (1, 1, 1, 1)])
    atom = o.system.shell_atom
    assert all(len({int(atom[i]) for i in b["shells"]}) == 4 for b in g["eri_blocks"])
    _check_eri_blocks(o, g)
    S, T, V, tab = o.overlap(), o.kinetic(), o.nuclear(), o.shell_table()
    assert sorted((tab[a][2], tab[b][2]) for a, b in (ob["shells"] for ob in g["one_electron_blocks"])) == [(2, 1), (3, 2), (3, 3)]
    for ob in g["one_electron_blocks"]:
        a, b = ob["shells"]
        assert atom[a] != atom[b]
        sl = (slice(tab[a][0], tab[a][0] + tab[a][1]), slice(tab[b][0], tab[b][0] + tab[b][1]))
        assert np.abs(S[sl] - np.array(ob["S"])).max() < 1e-13
        assert np.abs(T[sl] - np.array(ob["T"])).max() < 1e-12
        assert np.abs(V[sl] - np.array(ob["V"])).max() < 1e-12


def test_oracle_f_quartets_beyond_the_boys_table_match_independent_implementation(skew_golden):
    """(f_A f_A|f_B f_B) and (d_A f_A|f_B d_B) at T = 59: Boys orders up to 12 from the asymptotic branch, not yet negligible."""
    from oracle.oracle import Oracle
    g = skew_golden["far"]
    m = syn.far(syn.far_distance(T_HIGH))[0]
    assert abs(syn.far_boys_argument(m) - g["boys_argument"]) < 1e-12 and g["boys_argument"] > BOYS_XMAX
    assert [b["L"] for b in g["eri_blocks"]] == [[3, 3, 3, 3], [2, 3, 3, 2]]
    _check_eri_blocks(Oracle(m), g)


def test_far_systems_sit_on_the_intended_sides_of_the_boys_switches():
    lo, hi = (syn.far_boys_argument(syn.far(syn.far_distance(T))[0]) for T in (T_LOW, T_HIGH))
    assert BOYS_SERIES_SWITCH < lo < BOYS_XMAX < hi
    assert abs(lo - T_LOW) < 1e-12 and abs(hi - T_HIGH) < 1e-12


def test_deep_keeps_more_primitive_pairs_than_a_packed_ket_entry_holds():
    m = syn.deep()[0]
    assert syn.same_centre_ket_primitives(m) == 169 > 127


@pytest.mark.parametrize("name", list(BUILDERS))
def test_host_model_matches_oracle_on_synthetic_systems(name):
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m, atoms = BUILDERS[name]()
    s, o = q.System(m), Oracle(m)
    n, nq = SIZES[name]
    assert s.n == o.n == m.n_basis() == n and s.n_quartets() == o.n_unique_quartets() == nq
    assert s.n_electrons() == len(atoms)
    assert abs(s.nuclear_repulsion() - o.nuclear_repulsion()) < 1e-13
    assert np.abs(s.overlap() - o.overlap()).max() < 1e-13
    assert np.abs(s.kinetic() - o.kinetic()).max() < 1e-12
    assert np.abs(s.nuclear() - o.nuclear()).max() < 1e-12
    # deterministic builders: a second call gives the same arrays
    m2 = BUILDERS[name]()[0]
    assert np.array_equal(m.exponents, m2.exponents) and np.array_equal(m.coefficients, m2.coefficients)
    assert np.array_equal(m.coordinates(), m2.coordinates())
    s.close()


@pytest.mark.parametrize("name", ["deep", "tetra-pure-2", "tetra-cart-2"])
def test_shard_plan_partitions_synthetic_systems(name):
    import qchem_rs_amd as q
    s = q.System(BUILDERS[name]()[0])
    seen = set()
    for r in range(3):
        qs = s.plan_shard_quartets(r, 3)
        assert s.plan_shard(r, 3)[0] == len(qs)
        for a, b, c, d in qs.tolist():
            assert a >= b and c >= d
            key = (a, b, c, d) if (a, b) >= (c, d) else (c, d, a, b)
            assert key not in seen
            seen.add(key)
    assert len(seen) == s.n_quartets() == SIZES[name][1]
    s.close()
