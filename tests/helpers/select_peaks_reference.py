"""NumPy restatement of what csrc/select_peaks_kernels.hip computes for one candidate peak, step by step (no GPU, no reference needed):
the window's normalisation, the Levenberg-Marquardt iteration of MINPACK's lmdif on the normal equations ("Peak
selection"), the 80th percentile of |fit - y| and the decision.  The sums are NumPy's, not the kernel's lane order, so parameters agree
with the kernel's to rounding, not bit for bit; decisions on the clear candidates of golden G32 agree with the reference's.

* :func:`fit_window`   (keep, [a, b, c, d, num, status], evaluations of the model) of one window
* ``jacobian="analytic"`` is the variant DESIGN.md reports on: the exact derivatives instead of forward differences (MINPACK's lmder).
"""
import numpy as np

MAX_EVALS = 1000                      # kFitMaxEvals: curve_fit's maxfev = 200 (4 + 1)
TOL = 1.49012e-8                      # kFitTol: curve_fit's ftol and xtol
STEP_EPS = 1.4901161193847656e-08     # kFitStepEps: sqrt(2^-52)
EPS = 2.220446049250313e-16
DWARF = 2.2250738585072014e-308
OK, SHORT, NOT_FINITE, CONSTANT, BUDGET, DIVERGED, GRADIENT = range(7)


def _chol(a):
    """The lower Cholesky factor of a symmetric 4 x 4 matrix, or None where it is not positive definite."""
    low = np.zeros((4, 4))
    for j in range(4):
        s = a[j, j] - (low[j, :j] ** 2).sum()
        if not (s > 0.0) or not np.isfinite(s):
            return None
        low[j, j] = np.sqrt(s)
        for i in range(j + 1, 4):
            low[i, j] = (a[i, j] - (low[i, :j] * low[j, :j]).sum()) / low[j, j]
    return low


def _forward(low, b):
    z = np.zeros(4)
    for i in range(4):
        z[i] = (b[i] - (low[i, :i] * z[:i]).sum()) / low[i, i]
    return z


def _backward(low, z):
    x = np.zeros(4)
    for i in range(3, -1, -1):
        x[i] = (z[i] - (low[i + 1:, i] * x[i + 1:]).sum()) / low[i, i]
    return x


def _step(h, g, diag, delta, par):
    """fit_step of the kernel: MINPACK's lmpar from the Cholesky factor of h + par D^2.  (par, p)."""
    low = _chol(h)
    parl = 0.0
    if low is not None:
        p = -_backward(low, _forward(low, g))
        dxnorm = np.linalg.norm(diag * p)
        fp = dxnorm - delta
        if fp <= 0.1 * delta:
            return 0.0, p
        z = _forward(low, diag * (diag * p) / dxnorm)
        parl = fp / (delta * (z * z).sum())
    else:
        p, dxnorm, fp = np.zeros(4), np.inf, np.inf
    gnorm = np.linalg.norm(g / diag)
    paru = gnorm / delta
    if paru == 0.0:
        paru = DWARF / min(delta, 0.1)
    par = min(max(par, parl), paru)
    if par == 0.0:
        par = gnorm / dxnorm
    for it in range(1, 11):
        if par == 0.0:
            par = max(DWARF, 0.001 * paru)
        low = _chol(h + par * np.diag(diag * diag))
        if low is None:
            par = par * 10.0
            continue
        p = -_backward(low, _forward(low, g))
        dxnorm = np.linalg.norm(diag * p)
        before = fp
        fp = dxnorm - delta
        if abs(fp) <= 0.1 * delta or (parl == 0.0 and fp <= before and before < 0.0) or it == 10:
            break
        z = _forward(low, diag * (diag * p) / dxnorm)
        parc = fp / (delta * (z * z).sum())
        if fp > 0.0:
            parl = max(parl, par)
        if fp < 0.0:
            paru = min(paru, par)
        par = max(parl, par + parc)
    return par, p


def fit_window(w, radius, tol, use_offset, jacobian="forward"):
    """One candidate whose window is `w` (the samples start .. stop of its row)."""
    w = np.asarray(w, np.float64)
    n = len(w)
    nan = [np.nan] * 5
    if n <= 3:
        return False, nan + [SHORT], 0
    if not np.isfinite(w).all():
        return False, nan + [NOT_FINITE], 0
    if w.min() == w.max():
        return False, nan + [CONSTANT], 0
    mean = w.sum() / n
    y = (w - w.min()) / np.sqrt(((w - mean) ** 2).sum() / n)
    xs = np.arange(n) - n // 2
    x = np.array([1.0, 1.0, 0.0, 0.0])

    def resid(q):
        t = (xs - q[2]) / (2 * (q[1] * q[1]))
        return q[0] * np.exp(-(t * t)) + q[3] - y

    with np.errstate(all="ignore"):
        r = resid(x)
        fnorm = np.sqrt((r * r).sum())
        nfev, par, delta, xnorm, first, diag, status = 1, 0.0, 0.0, 0.0, True, np.ones(4), BUDGET
        while status == BUDGET and nfev < MAX_EVALS:
            r = resid(x)
            if jacobian == "forward":
                cols = []
                for j in range(4):
                    h = STEP_EPS * abs(x[j])
                    if h == 0.0:
                        h = STEP_EPS
                    xh = x.copy()
                    xh[j] += h
                    cols.append((resid(xh) - r) / h)
                jac = np.stack(cols, axis=1)
                nfev += 4
            else:
                t = (xs - x[2]) / (2 * (x[1] * x[1]))
                e = np.exp(-(t * t))
                jac = np.stack([e, 4 * x[0] * e * t * t / x[1], x[0] * e * t / (x[1] * x[1]), np.ones(n)], axis=1)
            h, g = jac.T @ jac, jac.T @ r
            if not (np.isfinite(np.diag(h)).all() and np.isfinite(g).all()):
                status = DIVERGED
                break
            colnorm = np.sqrt(np.diag(h))
            if first:
                diag = np.where(colnorm == 0.0, 1.0, colnorm)
                xnorm = np.linalg.norm(diag * x)
                delta = 100.0 * xnorm if xnorm != 0.0 else 100.0
            if fnorm == 0.0 or np.abs(g).max() == 0.0:
                status = OK
                break
            gnorm = max([abs(g[j] / (fnorm * colnorm[j])) for j in range(4) if colnorm[j] != 0.0], default=0.0)
            if gnorm <= EPS:
                status = GRADIENT
                break
            diag = np.maximum(diag, colnorm)
            while True:
                par, p = _step(h, g, diag, delta, par)
                if not np.isfinite(p).all():
                    status = DIVERGED
                    break
                xn = x + p
                pnorm = np.linalg.norm(diag * p)
                if first:
                    delta, first = min(delta, pnorm), False
                rn = resid(xn)
                nfev += 1
                fnorm1 = np.sqrt((rn * rn).sum())
                if not np.isfinite(fnorm1):
                    fnorm1 = np.inf
                actred = 1.0 - (fnorm1 / fnorm) ** 2 if 0.1 * fnorm1 < fnorm else -1.0
                temp1 = np.sqrt(max(p @ (h @ p), 0.0)) / fnorm
                temp2 = np.sqrt(par) * pnorm / fnorm
                prered = temp1 * temp1 + temp2 * temp2 / 0.5
                dirder = -(temp1 * temp1 + temp2 * temp2)
                ratio = actred / prered if prered != 0.0 else 0.0
                if ratio <= 0.25:
                    temp = 0.5 if actred >= 0.0 else 0.5 * dirder / (dirder + 0.5 * actred)
                    if 0.1 * fnorm1 >= fnorm or temp < 0.1:
                        temp = 0.1
                    delta = temp * min(delta, pnorm / 0.1)
                    par = par / temp
                elif par == 0.0 or ratio >= 0.75:
                    delta = pnorm / 0.5
                    par = 0.5 * par
                if ratio >= 1e-4:
                    x = xn
                    xnorm = np.linalg.norm(diag * x)
                    fnorm = fnorm1
                if abs(actred) <= TOL and prered <= TOL and 0.5 * ratio <= 1.0:
                    status = OK
                if delta <= TOL * xnorm:
                    status = OK
                if status == OK or ratio >= 1e-4 or nfev >= MAX_EVALS:
                    break
        if status == OK and not (np.isfinite(x).all() and np.isfinite(fnorm)):
            status = DIVERGED
        if status != OK:
            return False, list(x) + [np.nan, status], nfev
        v = np.sort(np.abs(resid(x)))
    pos = 0.8 * (n - 1)
    k = int(pos)
    num = v[k] + (pos - k) * (v[min(k + 1, n - 1)] - v[k])
    keep = abs(x[2]) < radius // 2 and num < tol and (not use_offset or abs(x[3]) < tol)
    return bool(keep), list(x) + [num, OK], nfev
