"""Batch-vectorised numpy model of crx_lqr_design (include/crx.h, L1..L4), written from the description there:

    P = Q
    repeat at most max_iter times:
        P' = A'PA - A'(PB) inv(R + B'(PB)) B'P A + Q
        if max|P' - P| < eps: stop, and discard P'
        P = P'
    K = inv(B'PB + R) B'P A

in the operation order of control._lqr_gain (every product left to right) and with the status table L4.  It runs in whatever
floating type `dtype` names (float64, numpy.longdouble).  The 2x2 inverse: `inverse="lapack"` is scipy.linalg.inv, what the
reference and control._lqr_gain call (float64 only; the default there, so that the model is the mirror bit for bit);
`inverse="plain"` is the adjugate over the determinant, what the kernel computes (the default for every other type).  The two
differ in the last bits only; whether a determinant counts as singular is decided on the plain determinant in both.

design() returns K [B,2,6], P [B,6,6], iters [B], status [B] and margin [B] = min over the steps of | max|P' - P| - eps | / eps:
how close the discrete stop decision of a car ever came to a tie (inf for a car that computed no step)."""
import numpy as np
import scipy.linalg as la

CONVERGED, MAX_ITER, SKIPPED, SINGULAR = 0, 1, 4, 6


def _T(M):
    return np.swapaxes(M, -1, -2)


def _inv2(G, inverse):
    """Inverse of a stack of 2x2 matrices; ok = the determinant is finite and non-zero."""
    a, b, c, d = G[:, 0, 0], G[:, 0, 1], G[:, 1, 0], G[:, 1, 1]
    with np.errstate(all="ignore"):
        det = a * d - b * c
        ok = np.isfinite(det) & (det != 0)
        safe = np.where(ok, det, 1)
        W = np.stack([np.stack([d / safe, -b / safe], axis=-1), np.stack([-c / safe, a / safe], axis=-1)], axis=-2)
    if inverse == "lapack":
        for i in np.flatnonzero(ok):
            try:
                W[i] = la.inv(G[i])
            except (la.LinAlgError, ValueError):
                ok[i] = False
    return W, ok


def riccati_step(A, B, Q, R, P, transposed_shortcut=False, inverse="plain"):
    """One step P -> P' for stacks A [B,6,6], B [B,6,2], P [B,6,6]; returns (P', ok).  transposed_shortcut: the variant L2 forbids,
    (B'P A)' in place of A'(PB)."""
    PB = P @ B
    G = R + _T(B) @ PB
    W, ok = _inv2(G, inverse)
    APB = _T(_T(B) @ P @ A) if transposed_shortcut else _T(A) @ PB
    nxt = _T(A) @ P @ A - APB @ W @ _T(B) @ P @ A + Q
    return nxt, ok


def gain(A, B, R, P, inverse="plain"):
    W, ok = _inv2(_T(B) @ P @ B + R, inverse)
    return W @ _T(B) @ P @ A, ok


def design(A, B, Q, R, max_iter=50, eps=0.01, dtype=np.float64, transposed_shortcut=False, inverse=None):
    if inverse is None:
        inverse = "lapack" if dtype is np.float64 else "plain"
    A = np.array(A, dtype=dtype).reshape(-1, 6, 6)
    B = np.array(B, dtype=dtype).reshape(-1, 6, 2)
    Q, R = np.array(Q, dtype=dtype).reshape(6, 6), np.array(R, dtype=dtype).reshape(2, 2)
    eps = dtype(eps)
    n = A.shape[0]
    P = np.repeat(Q[None], n, axis=0)
    iters = np.zeros(n, dtype=np.int32)
    status = np.full(n, MAX_ITER, dtype=np.int32)
    margin = np.full(n, np.inf)
    sing = ~(np.isfinite(A).all(axis=(1, 2)) & np.isfinite(B).all(axis=(1, 2)))   # L4: a non-finite model computes no step
    run = ~sing
    with np.errstate(all="ignore"):
        for _ in range(int(max_iter)):
            if not run.any():
                break
            j = np.flatnonzero(run)
            iters[j] += 1
            nxt, ok = riccati_step(A[j], B[j], Q, R, P[j], transposed_shortcut, inverse)
            ok &= np.isfinite(nxt).all(axis=(1, 2))
            diff = np.abs(nxt - P[j]).max(axis=(1, 2))
            good = j[ok]
            margin[good] = np.minimum(margin[good], (np.abs(diff[ok] - eps) / eps).astype(np.float64))
            passed = ok & (diff < eps)                   # L3: strict
            sing[j[~ok]] = True
            status[j[passed]] = CONVERGED                # L1: the passing iterate is discarded
            go = ok & ~passed
            P[j[go]] = nxt[go]
            run[j[~go]] = False
        K, ok = gain(A, B, R, P, inverse)
        sing |= ~ok | ~np.isfinite(K).all(axis=(1, 2))
    K[sing], P[sing] = np.nan, np.nan
    status[sing] = SINGULAR
    return dict(K=K, P=P, iters=iters, status=status, margin=margin)


def step(K, x, xt):
    """u = -K (x - xt) for stacks K [B,2,6], x, xt [B,6]."""
    return -(K @ (np.asarray(x) - np.asarray(xt))[..., None])[..., 0]


def draw_models(rng, A0, B0, n, scales=(1e-3, 1e-2, 5e-2)):
    """Generator G: n models A0 (1 + s z), B0 (1 + s z), z standard normal per entry, s dealt round-robin from `scales`.
    Returns A [n,6,6], B [n,6,2], s [n]."""
    s = np.array([scales[i % len(scales)] for i in range(n)])
    A = A0[None] * (1 + s[:, None, None] * rng.standard_normal((n, 6, 6)))
    B = B0[None] * (1 + s[:, None, None] * rng.standard_normal((n, 6, 2)))
    return A, B, s
