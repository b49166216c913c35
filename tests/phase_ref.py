"""Plain NumPy restatement of the phase-curve definition (the header comment of frei_phs_apply in
include/frei_hip.h), written from the definition alone: explicit loops over the phase p and the
cell c in the stated order, vectorised over wavelength only.  The checker of
tests/test_gpu_phase.py, itself pinned by tests/test_phasecurve_host.py; it imports
tests/emergent_ref.py (the intensity of one column at one angle) and nothing of the package under
test."""
import numpy as np

from tests import emergent_ref as R


def visible(mu):
    """The pairs (p, c) the sum takes: exactly those with mu > 0."""
    return np.asarray(mu, dtype=float) > 0.0


def phase_curve(dtaus, T, lam_um, select, mu, coef):
    """out[n_phase][n_lam]: ``dtaus`` [n_atm][n_layers][n_lam], ``T`` [n_atm][n_layers],
    ``select`` [n_cell], ``mu`` and ``coef`` [n_phase][n_cell].  Per phase the visible cells in
    ascending c; the first term starts the sum, every later one enters as acc + coef * I; a
    phase that sees nothing gives 0.  The coef of an invisible pair is never read."""
    dtaus = np.asarray(dtaus, dtype=float)
    T = np.asarray(T, dtype=float)
    mu = np.asarray(mu, dtype=float)
    coef = np.asarray(coef, dtype=float)
    n_phase, n_cell = mu.shape
    out = np.zeros((n_phase, dtaus.shape[-1]))
    for p in range(n_phase):
        acc = None
        for c in range(n_cell):
            if not mu[p, c] > 0.0:
                continue
            m = int(select[c])
            inten, _ = R.emergent(dtaus[m], T[m], lam_um, np.array([mu[p, c]]))
            term = coef[p, c] * inten[0]
            acc = term if acc is None else acc + term
        if acc is not None:
            out[p] = acc
    return out


def accumulate(intensity_of, select, mu, coef, n_lam):
    """The same sum over intensities the caller supplies: ``intensity_of(m, mu_pc)`` -> [n_lam]
    (the bitwise check feeds it the device's own frei_emergent intensities)."""
    mu = np.asarray(mu, dtype=float)
    coef = np.asarray(coef, dtype=float)
    out = np.zeros((mu.shape[0], n_lam))
    for p in range(mu.shape[0]):
        acc = None
        for c in range(mu.shape[1]):
            if not mu[p, c] > 0.0:
                continue
            term = coef[p, c] * intensity_of(int(select[c]), mu[p, c])
            acc = term if acc is None else acc + term
        if acc is not None:
            out[p] = acc
    return out
