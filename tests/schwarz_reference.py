"""Reference side of the Schwarz tests (test_schwarz_host.py, test_schwarz_gpu.py): factors, working thresholds, predicted kept sets
and masks - all from the oracle's dense tensor, nothing from the library under test.

  pair_factors(o, I)       Q_ref[(a, b)] = sqrt(max over the diagonal of the (ab|ab) block of I), every shell pair a >= b
  working_tau(prod, nom)   the threshold the tests use near a nominal one: the geometric middle of the widest gap between consecutive
                           sorted products Q_P Q_Q within a decade either side of it, with the gap's ratio - a decision `product >= tau`
                           then cannot depend on the last bits of a factor
  predicted(...)           the unique quartets the screening rule keeps, as sorted (a, b, c, d) tuples with pair (a, b) >= pair (c, d)
  function_mask(...)       mask[i, j, k, l] = Qf[i, j] Qf[k, l] >= tau, Qf = Q_ref spread over function pairs"""
import numpy as np

NOMINAL_TAUS = (1e-12, 1e-9, 1e-6, 1e-3)


def pair_factors(o, I):
    tab = o.shell_table()
    Q = {}
    for a in range(len(tab)):
        for b in range(a + 1):
            sa, sb = slice(tab[a][0], tab[a][0] + tab[a][1]), slice(tab[b][0], tab[b][0] + tab[b][1])
            blk = I[sa, sb, sa, sb].reshape(tab[a][1] * tab[b][1], -1)
            Q[(a, b)] = float(np.sqrt(np.diag(blk).max()))
    return Q


def pair_list(Q):
    """the shell pairs in the library's order: a ascending, b <= a ascending"""
    return sorted(Q)


def quartet_products(Q, pairs=None):
    """Q_P Q_Q of every unique quartet P >= Q of `pairs` (default: all), with the index arrays (P, Q) into the pair list"""
    pl = pair_list(Q) if pairs is None else list(pairs)
    q = np.array([Q[p] for p in pl])
    P, K = np.tril_indices(len(pl))
    return q[P] * q[K], P, K, pl


def working_tau(products, nominal):
    """(tau, ratio of the gap it sits in)"""
    s = np.sort(products[(products >= nominal / 10) & (products <= nominal * 10)])
    assert len(s) >= 2, nominal
    r = s[1:] / s[:-1]
    k = int(np.argmax(r))
    return float(np.sqrt(s[k] * s[k + 1])), float(r[k])


def canonical(a, b, c, d):
    return (a, b, c, d) if (a, b) >= (c, d) else (c, d, a, b)


def predicted(Q, tau, stored):
    """sorted unique quartets among the `stored` pairs with Q_P Q_Q >= tau (tau = 0: all of them)"""
    prod, P, K, pl = quartet_products(Q, sorted(stored))
    keep = prod >= tau
    return sorted(pl[p] + pl[k] for p, k in zip(P[keep], K[keep]))


def function_factors(o, Q):
    tab = o.shell_table()
    Qf = np.zeros((o.n, o.n))
    for (a, b), v in Q.items():
        sa, sb = slice(tab[a][0], tab[a][0] + tab[a][1]), slice(tab[b][0], tab[b][0] + tab[b][1])
        Qf[sa, sb] = v
        Qf[sb, sa] = v
    return Qf


def function_mask(Qf, tau):
    return (Qf[:, :, None, None] * Qf[None, None, :, :]) >= tau
