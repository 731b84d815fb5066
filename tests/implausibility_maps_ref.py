"""NumPy restatement of the maps over a mesh of two inputs (gpe_hm_cells) and of the explicit rows
they stand for (test infrastructure, NumPy only).

Candidate s = (i g2 + j) ns + t has x1[i] in column ca, x2[j] in column cb and others[t] in the
remaining columns in ascending order: the array imp_plot builds.  Level l of a candidate is the
(l + 1)-th largest sqrt(I^2) over the outputs, a NaN above every number; per cell IMP is the
level's minimum over the ns samples (NaN if any is NaN) and ``below`` the number of samples
with the level < cm."""
import numpy as np

from implausibility_ref import imaxes


def cell_rows(D, ca, cb, x1, x2, others):
    """The (g1 g2 ns) x D explicit rows, by loops."""
    x1, x2 = np.asarray(x1, dtype=float), np.asarray(x2, dtype=float)
    others = np.asarray(others, dtype=float)
    ns = others.shape[0]
    others = others.reshape(ns, D - 2)
    rest = [k for k in range(D) if k not in (ca, cb)]
    x = np.empty((x1.size * x2.size * ns, D))
    s = 0
    for a in x1:
        for b in x2:
            for t in range(ns):
                x[s, ca], x[s, cb] = a, b
                x[s, rest] = others[t]
                s += 1
    return x


def maps(I2, cells, ns, maxno, cm, use=None):
    """(imp, below), each maxno x cells, from I^2 (cells ns x outputs); an output whose flag of
    ``use`` is off enters as a zero column."""
    I2 = np.array(I2, dtype=float)
    if use is not None:
        I2[:, ~np.asarray(use, dtype=bool)] = 0.0
    top = imaxes(I2, maxno).reshape(cells, ns, maxno)
    imp = np.empty((maxno, cells))
    below = np.zeros((maxno, cells), dtype=np.int64)
    for l in range(maxno):
        for c in range(cells):
            col = top[c, :, maxno - 1 - l]
            imp[l, c] = np.nan if np.any(np.isnan(col)) else min(col)
            below[l, c] = sum(1 for v in col if v < cm)
    return imp, below
