"""NumPy restatement of the EM refinement of the M x M spatial filter of the microphone-array path (include/gccnmf_array_em.h,
csrc/array_spatial_em.hip): the M-channel form of tests/spatial_em_restatement.py (EM), built on tests/array_spatial_restatement.py
(AS: ldl_solve, apply_row, hermitian).  Per file, E[i, c] the ratio-mode estimates (S, M, F, T), X (M, F, T), lambda = AS.LOADING:

    start      v_i = AS.powers(E),  R~_i = AS.covariances(E)
    iteration  for every bin, against the OLD R~:  Sigma = sum_j v_j R~_j,  G_i = v_i R~_i Sigma^-1,  s_i = G_i X,
               C_i = s_i s_i^H + (I - G_i) v_i R~_i,  v'_i = max(0, (1/M) Re tr(R~_i^-1 C_i)),  v'_i = 0 for every i where sum_j v_j = 0;
               then  A_i = sum over the frames with v'_i != 0 of C_i / v'_i (float32 terms, float64 sum),  n_i = their number,
               R'_i = A_i / n_i (I when n_i = 0),  R~'_i = R'_i + lambda (tr R'_i / M) I, rounded to float32 once;  v <- v', R~ <- R~'
    output     v_i R~_i Sigma^-1 X, the filter's formulas on the final v and R~  (``filter_with``)

``em_step`` evaluates the cancellation-free form the header states (k_i = Re tr(Z N_i), P_i = R~_i (Z N_i), no inverse of R~_i), in both
precisions through the same lines, so that their distance is what float32 costs and nothing else: float32 runs the header's order operation
by operation on w_j = v_j 2^-e with the frame sums in the device's order (spatial_checks.device_sum) and is meant to equal the device bit
for bit; float64 (e = 0, frames ascending) is the contract.  ``literal_step`` evaluates the definition as written, with numpy.linalg.inv;
tests/test_array_em_host.py holds the two together.  At M = 2 everything here is EM's (as the device runs spatial_em_frame there).
The keywords ``divisor``, ``loading`` and ``count`` plant mistakes.  Nothing here knows about the device."""
import numpy as np

import array_spatial_restatement as AS
import spatial_checks as SC
import spatial_em_restatement as EM
import spatial_restatement as SR

LOADING = AS.LOADING
BAR_FACTOR = SR.BAR_FACTOR


def _row(R, j, F):
    """The M M stored components of target j's R~ as (F, 1) columns."""
    return [R[j, :, g].reshape(F, 1) for g in range(R.shape[-1])]


def _sigma(w, r, S, MM):
    sg = []
    for g in range(MM):
        a = w[0] * r[0][g]
        for j in range(1, S):
            a = a + w[j] * r[j][g]
        sg.append(a)
    return sg


def _scale(v, dtype, scaled):
    """-> (w, e, vs): AS._scaled where the evaluation is the scaled one; e = 0 otherwise."""
    if scaled:
        w, vs = AS._scaled(v)
        fin = np.isfinite(vs)
        e = np.where(fin, np.frexp(np.where(fin, vs, 0))[1], 0)
        return w.astype(dtype), e, vs
    vs = v[0].copy()
    for j in range(1, v.shape[0]):
        vs = vs + v[j]
    return v, np.zeros(v.shape[1:], np.int64), vs


def filter_with(v, R, X, dtype=np.float64, scaled=None):
    """The output stage on given powers v (S, F, T) and covariance rows R (S, F, M M): AS.spatial_filter(E, X, np.float32, R=R)'s bits
    when v = AS.powers(E, np.float32); both precisions run the header's LDL^H order."""
    R = np.asarray(R, np.float32)
    X = np.asarray(X).astype(np.complex64)
    M = X.shape[0]
    if M == 2:
        return EM.filter_with(v, R, X, dtype, scaled)
    v = np.asarray(v, dtype)
    S, F, T = v.shape
    MM = M * M
    if scaled is None:
        scaled = dtype == np.float32
    Rd = R.astype(dtype)
    out = np.zeros((S, M, F, T), np.complex128 if dtype == np.float64 else np.complex64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        w, _, vs = _scale(v, dtype, scaled)
        r = [_row(Rd, j, F) for j in range(S)]
        xr, xi = [X[c].real.astype(dtype) for c in range(M)], [X[c].imag.astype(dtype) for c in range(M)]
        yr, yi, _ = AS.ldl_solve(_sigma(w, r, S, MM), xr, xi, M)
        for i in range(S):
            for a in range(M):
                ur, ui = AS.apply_row(r[i], a, yr, yi, M)
                out[i, a].real, out[i, a].imag = w[i] * ur, w[i] * ui
    out[:, :, vs == 0] = 0
    return out


def em_step(v, R, X, dtype=np.float64, scaled=None, frame_sum=None, divisor=None, loading='trace', count='used'):
    """One iteration.  v (S, F, T) in dtype, R (S, F, M M) float32 -> (v' in dtype, R~' float32).  ``frame_sum`` (float64 (F, T) -> (F,))
    replaces the order in which the frames' terms are added.  Planted mistakes: divisor (v" divided by it instead of M), loading='lambda'
    (the loading without the trace), count='all' (every frame counted in n_i)."""
    X = np.asarray(X).astype(np.complex64)
    M = X.shape[0]
    if M == 2 and divisor is None and loading == 'trace' and count == 'used':
        if frame_sum is None and dtype == np.float32:
            frame_sum = SC.device_sum
        return EM.em_step(v, R, X, dtype, scaled, frame_sum=frame_sum)
    v = np.asarray(v, dtype)
    S, F, T = v.shape
    MM = M * M
    Rd = np.asarray(R, np.float32).astype(dtype)
    if scaled is None:
        scaled = dtype == np.float32
    if frame_sum is None:
        frame_sum = SC.device_sum if dtype == np.float32 else SC.ascending_sum
    vn = np.zeros_like(v)
    Rn = np.zeros((S, F, MM), np.float64)
    zero = np.zeros((F, T), dtype)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        w, e, vs = _scale(v, dtype, scaled)
        r = [_row(Rd, j, F) for j in range(S)]
        sg = _sigma(w, r, S, MM)
        # N_i = sum_{j != i} w_j R~_j, ascending j: zeros at S = 1
        N = []
        for i in range(S):
            comp = []
            for g in range(MM):
                a = None
                for j in range(S):
                    if j != i:
                        a = w[j] * r[j][g] if a is None else a + w[j] * r[j][g]
                comp.append(zero if a is None else a)
            N.append(comp)
        # one factorisation, 1 + S M right-hand sides: X and the columns of every N_i, stacked in front of (F, T)
        rhs_r, rhs_i = [], []
        for c in range(M):
            pr, pi = [X[c].real.astype(dtype)], [X[c].imag.astype(dtype)]
            for i in range(S):
                for b in range(M):
                    if c == b:
                        pr.append(N[i][b] + zero)
                        pi.append(zero)
                    elif c < b:
                        q = M + 2 * AS.pair_index(M, c, b)
                        pr.append(N[i][q] + zero)
                        pi.append(N[i][q + 1] + zero)
                    else:
                        q = M + 2 * AS.pair_index(M, b, c)
                        pr.append(N[i][q] + zero)
                        pi.append(-N[i][q + 1] + zero)
            rhs_r.append(np.stack(pr))
            rhs_i.append(np.stack(pi))
        sol_r, sol_i, _ = AS.ldl_solve(sg, rhs_r, rhs_i, M)
        yr, yi = [s[0] for s in sol_r], [s[0] for s in sol_i]
        for i in range(S):
            ur, ui, h = [], [], None
            for a in range(M):
                tr, ti = AS.apply_row(r[i], a, yr, yi, M)
                ur.append(tr)
                ui.append(ti)
                q = yr[a] * tr + yi[a] * ti
                h = q if a == 0 else h + q
            P, k = [None] * MM, None
            for b in range(M):
                wr, wi = [s[1 + i * M + b] for s in sol_r], [s[1 + i * M + b] for s in sol_i]
                k = wr[b] if b == 0 else k + wr[b]
                for a in range(b + 1):
                    pr, pi = AS.apply_row(r[i], a, wr, wi, M)
                    if a == b:
                        P[a] = pr
                    else:
                        q = M + 2 * AS.pair_index(M, a, b)
                        P[q], P[q + 1] = pr, pi
            v2 = (w[i] * h + np.ldexp(k, e).astype(dtype)) / dtype(M if divisor is None else divisor)
            vi = w[i] * v2
            vi = np.where(vi < 0, dtype(0), vi)
            vi[vs == 0] = 0
            vn[i] = vi
            rv = dtype(1.0) / v2
            c = [(w[i] * (ur[a] * ur[a] + ui[a] * ui[a]) + np.ldexp(P[a], e).astype(dtype)) * rv for a in range(M)]
            for a, b in AS.pairs(M):
                q = M + 2 * AS.pair_index(M, a, b)
                c.append((w[i] * (ur[a] * ur[b] + ui[a] * ui[b]) + np.ldexp(P[q], e).astype(dtype)) * rv)
                c.append((w[i] * (ui[a] * ur[b] - ur[a] * ui[b]) + np.ldexp(P[q + 1], e).astype(dtype)) * rv)
            use = ~(vi == 0)                                   # NaN counts
            sums = [frame_sum(np.where(use, ck, 0).astype(np.float64)) for ck in c]
            cnt = (use.sum(axis=-1) if count == 'used' else np.full(F, T)).astype(np.float64)
            none = cnt == 0
            den = np.where(none, 1.0, cnt)
            d = [np.where(none, 1.0, sums[a] / den) for a in range(M)]
            tr = d[0]
            for a in range(1, M):
                tr = tr + d[a]
            load = LOADING * (tr / float(M)) if loading == 'trace' else LOADING
            Rn[i] = np.stack([d[a] + load for a in range(M)] + [np.where(none, 0.0, sums[g] / den) for g in range(M, MM)], axis=-1)
    return vn, Rn.astype(np.float32)


def literal_step(v, R, X):
    """One iteration as the definition is written, float64 with complex M x M matrices and numpy.linalg.inv: (v', R'_i before the loading
    and the rounding, as (S, F, M, M) complex)."""
    v = np.asarray(v, np.float64)
    S, F, T = v.shape
    X = np.asarray(X).astype(np.complex64).astype(np.complex128)
    M = X.shape[0]
    Rm = AS.hermitian(np.asarray(R, np.float32).astype(np.float64), M)                                  # (S, F, M, M)
    Xv = np.moveaxis(X, 0, -1)[..., None]                                                              # (F, T, M, 1)
    Sigma = (v[..., None, None] * Rm[:, :, None]).sum(axis=0)                                          # (F, T, M, M)
    live = v.sum(axis=0) != 0
    Si = np.linalg.inv(np.where(live[..., None, None], Sigma, np.eye(M)))
    vn, Rn = np.zeros_like(v), np.zeros((S, F, M, M), np.complex128)
    for i in range(S):
        vR = v[i][..., None, None] * Rm[i][:, None]
        G = vR @ Si
        s = G @ Xv
        C = s @ np.conj(np.swapaxes(s, -1, -2)) + (np.eye(M) - G) @ vR
        vi = np.maximum(0.0, np.trace(np.linalg.inv(Rm[i])[:, None] @ C, axis1=-2, axis2=-1).real / M)
        vi[~live] = 0
        vn[i] = vi
        use = vi != 0
        A = np.where(use[..., None, None], C / np.where(use, vi, 1.0)[..., None, None], 0).sum(axis=1)
        cnt = use.sum(axis=1)
        Rn[i] = np.where((cnt == 0)[:, None, None], np.eye(M), A / np.maximum(cnt, 1)[:, None, None])
    return vn, Rn


def refine(E, X, n, dtype=np.float64, R=None, cache=None, **variant):
    """-> (v, R~) after n iterations: (S, F, T) in dtype, (S, F, M M) float32.  R: the start's covariance rows instead of
    AS.covariances(E, frame_sum=...) -- float32: the device's order; float64: ascending.  cache: a dict that keeps the state after every
    iteration under (dtype, m), so that a later call for the same E and X goes on from the nearest one."""
    m, v = 0, None
    if cache is not None:
        for k in range(int(n), -1, -1):
            if (dtype, k) in cache:
                m, (v, R) = k, cache[(dtype, k)]
                break
    if v is None:
        if R is None:
            R = AS.covariances(E, frame_sum=SC.device_sum if dtype == np.float32 else None)
        v = AS.powers(E, dtype)
    for k in range(m, int(n)):
        v, R = em_step(v, R, X, dtype, **variant)
        if cache is not None:
            cache[(dtype, k + 1)] = (v, R)
    return v, R


def array_em(E, X, n, dtype=np.float64, **variant):
    """E (S, M, F, T), X (M, F, T) -> E' (S, M, F, T) after n iterations; n = 0 is AS.spatial_filter(E, X, dtype)."""
    if not int(n):
        return AS.spatial_filter(E, X, dtype)
    v, R = refine(E, X, n, dtype, **variant)
    return filter_with(v, R, X, dtype)


def measured_bar(E, X, n):
    """(bar, float32 error, E' float64, (v32, R32, out32)): BAR_FACTOR times the float32-to-float64 distance of the restatement relative
    to max|X|, as EM.measured_bar.  The condition the bar rests on is asserted: the zero pattern of the powers and the NaN pattern are the
    same in the two evaluations."""
    X = np.asarray(X)
    v64, R64 = refine(E, X, n, np.float64)
    v32, R32 = refine(E, X, n, np.float32)
    assert np.array_equal(v64 == 0, v32 == 0), 'the zero pattern of the powers differs between float32 and float64'
    assert np.array_equal(np.isnan(v64), np.isnan(v32)) and np.array_equal(np.isnan(R64), np.isnan(R32))
    ref = filter_with(v64, R64, X, np.float64) if int(n) else AS.spatial_filter(E, X, np.float64)
    f32 = filter_with(v32, R32, X, np.float32) if int(n) else AS.spatial_filter(E, X, np.float32)
    assert np.array_equal(np.isfinite(ref), np.isfinite(f32))
    ok = np.isfinite(ref)
    scale = float(np.abs(X[np.isfinite(X)]).max())
    err = float(np.abs(f32[ok] - ref[ok]).max()) / scale if ok.any() else 0.0
    return BAR_FACTOR * err, err, ref, (v32, R32, f32)
