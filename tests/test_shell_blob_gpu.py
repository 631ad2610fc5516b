"""The shell blob of a handle (shells, primitives, transforms, nuclei on the device) is uploaded by whichever call needs it first -
the one-electron kernel or the gradient.  Who came first must not show in a single bit of either."""
import numpy as np
import pytest

from conftest import data
from synthetic_systems import BUILDERS, rand_sym

pytestmark = pytest.mark.gpu


def _water():
    import qchem_rs_amd as q
    return q.MolecularSystem.load(data("mol", "water.json"), q.BasisSet.load(data("basis", "6-31G_st_st.json")))      # s, p, d; n = 25


SYSTEMS = {"water-631gss": _water, "far-40": lambda: BUILDERS["far-40"]()[0]}                # far-40: the smallest builder with f shells (n = 32)


@pytest.fixture(scope="module", params=sorted(SYSTEMS))
def runs(request):
    """the same (D, W) on two fresh handles: gradient first / one-electron matrices first, then the gradient, then the matrices again"""
    import qchem_rs_amd as q
    m = SYSTEMS[request.param]()
    a, b = q.System(m), q.System(m)
    D, W = rand_sym(a.n, 11), rand_sym(a.n, 12)
    g_first = np.stack(a.gradient(D, W))
    stv_before = [b.one_electron_gpu(w) for w in range(3)]
    g_second = np.stack(b.gradient(D, W))
    stv_after = [b.one_electron_gpu(w) for w in range(3)]
    a.close(); b.close()
    return g_first, g_second, stv_before, stv_after


def test_gradient_does_not_depend_on_who_uploaded_the_blob(runs):
    g_first, g_second, _, _ = runs
    assert np.all(np.isfinite(g_first)) and np.abs(g_first[1:]).max() > 0.0
    assert g_first.tobytes() == g_second.tobytes()


def test_one_electron_matrices_unchanged_by_a_gradient_between(runs):
    _, _, before, after = runs
    for w in range(3):
        assert np.abs(before[w]).max() > 0.0
        assert before[w].tobytes() == after[w].tobytes()
