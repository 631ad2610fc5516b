"""CPU tests behind test_schwarz_gpu.py: how well the oracle knows the Schwarz factors, and the stretched system the screening tests run on.

The factors of spread() go down to 7e-42, so the GPU's factors are judged by a RELATIVE bar, and a relative bar needs a reference
whose own relative error is known.  tests/golden/schwarz_golden.json (tools/gen_golden.py schwarz) holds sqrt(max_ab (ab|ab)) of every
shell pair of spread() and deep() from the independent numpy/scipy implementation, and for the ss pairs a second value from the closed
form in mpmath at 50 digits.  Measured here (printed by the test), over pairs with Q >= 1e-150:

    oracle against eri_block        spread 6.50e-16 (91 pairs)   deep 1.04e-14 (28 pairs)
    oracle against the closed form  spread 1.36e-15 (15 pairs)   deep 5.55e-15 (6 pairs)

(deep's 13-primitive shells sum 28 561 primitive quartets per pair.)  ORACLE_VS_GOLDEN is the largest of these; the bar of the GPU
test is 100 times it (the kernels sum in another order), floored at 1e-13 relative (a reference that happens to agree to the last bit
proves nothing about the next system): SCHWARZ_BAR = 1.04e-12."""
import json
import os

import numpy as np
import pytest

import schwarz_reference as sr
import synthetic_systems as syn
from conftest import ROOT

ORACLE_VS_GOLDEN = 1.04e-14
SCHWARZ_BAR = max(100 * ORACLE_VS_GOLDEN, 1e-13)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "schwarz_golden.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["spread", "deep"])
def test_oracle_schwarz_factors_match_both_independent_columns(golden, name):
    from oracle.oracle import Oracle
    m = syn.BUILDERS[name]()[0]
    o = Oracle(m)
    Q = sr.pair_factors(o, syn.oracle_tensor(o))
    g = golden[name]
    assert [tuple(p) for p in g["pairs"]] == sr.pair_list(Q) and len(Q) == m.n_shells * (m.n_shells + 1) // 2
    L = m.shell_L
    assert [tuple(p) for p in g["ss_pairs"]] == [p for p in sr.pair_list(Q) if L[p[0]] == 0 and L[p[1]] == 0] and g["ss_pairs"]
    worst = {}
    for col, pairs, ref in (("eri_block", g["pairs"], g["Q"]), ("closed form", g["ss_pairs"], g["ss_Q_closed_form"])):
        rel = [abs(Q[tuple(p)] - r) / r for p, r in zip(pairs, ref) if r >= 1e-150]
        assert len(rel) == len(pairs)                  # (nothing of these systems is below 1e-150: every pair is compared)
        worst[col] = max(rel)
        print("%s: oracle against %s, largest relative disagreement of a Schwarz factor %.2e over %d pairs (Q from %.1e to %.1e)"
              % (name, col, worst[col], len(rel), min(ref), max(ref)))
    assert max(worst.values()) <= ORACLE_VS_GOLDEN, worst
    assert SCHWARZ_BAR == max(100 * ORACLE_VS_GOLDEN, 1e-13)


def test_schwarz_factor_accessor_is_declared_and_never_answers_without_a_device():
    """qc_schwarz_factors: in the header, in the symbol list of hf.py, refuses a null handle; the factors come from a device pass, so
    without a gfx950 device the call is an error (there is no host fallback), with one it returns one factor per stored pair"""
    import qchem_rs_amd as q
    L = q.lib()
    header = open(os.path.join(ROOT, "include", "qchem_hip.h")).read()
    assert "int qc_schwarz_factors(qc_system *sys, int32_t *shell_ab, double *Q, int64_t capacity);" in header
    assert "qc_schwarz_factors" in q.hf.EXPORTS and hasattr(L, "qc_schwarz_factors")
    assert L.qc_schwarz_factors(None, None, None, 0) == q.hf.QC_ERR_INVALID
    s = q.System(syn.spread()[0])
    if q.device_ready():
        ab, Q = s.schwarz_factors()
        assert len(ab) == len(Q) > 0 and np.all(ab[:, 0] >= ab[:, 1])
    else:
        with pytest.raises(q.hf.QcError, match="no gfx950 device"):
            s.schwarz_factors()
    s.close()


def test_spread_is_the_system_the_screening_tests_need():
    """What test_schwarz_gpu.py relies on, on the reference alone: the range of the factors, the Schwarz inequality itself, working
    thresholds in gaps of at least 5 % that drop between 30 % and 95 % of the quartets, pairs below the primitive cut-off."""
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m = syn.spread()[0]
    o = Oracle(m)
    I = syn.oracle_tensor(o)
    Q = sr.pair_factors(o, I)
    vals = np.array(list(Q.values()))
    assert o.n == 37 and len(Q) == 91 and vals.min() < 1e-40 and 1.3 < vals.max() < 1.4
    Qf = sr.function_factors(o, Q)
    bound = Qf[:, :, None, None] * Qf[None, None, :, :]
    assert np.all(np.abs(I) <= bound * (1 + 1e-14) + 1e-300)
    prod = sr.quartet_products(Q)[0]
    assert len(prod) == 4186
    for nominal in sr.NOMINAL_TAUS:
        tau, ratio = sr.working_tau(prod, nominal)
        share = float(np.mean(prod < tau))
        print("nominal %.0e: working tau %.4e, gap ratio %.3f, %.1f %% dropped" % (nominal, tau, ratio, 100 * share))
        assert nominal / 10 <= tau <= nominal * 10 and ratio >= 1.05 and 0.30 <= share <= 0.95
    # the host model stores fewer pairs than there are: the pair index of the library is not the triangular index
    s = q.System(m)
    qs = s.plan_shard_quartets(0, 1)
    stored = {(a, b) for a, b, _, _ in qs.tolist()} | {(c, d) for _, _, c, d in qs.tolist()}
    assert 0 < len(stored) < 91 and len(qs) == len(stored) * (len(stored) + 1) // 2
    s.close()
