"""BSS Eval 3.0 image criteria (`bss_eval_images`: Vincent, Sawada, Bofill, Makino & Rosca 2007) on the device -- SDR, ISR, SIR and SAR
with time-invariant distortion filters of ``filterLength`` taps, per file of a batch.

The device part is two HIP kernels of libgccnmf_eval.so (csrc/bss_eval.hip, bound by ``_eval``): the lag correlations of the true source
images with each other and with the estimates, which are the block-Toeplitz Gram matrix and the right-hand sides of the projections, and
the projections themselves (FIR sums with float64 coefficients).  Between them torch does the plumbing in float64 on the device: the
Toeplitz expansion (indexing), the solves (batched LU, ``torch.linalg.solve_ex``: the float64 Cholesky of the torch build this was measured
on is not reliable, see ``_solve``) and the seven energy sums per (estimate, source) pair (``torch.sum``).  There is NO CPU fallback: ``HipLibraryError`` without the
library or a device.

Definition, for true images s[i][c][n] and estimates e[j][c][n], zero outside [0, n), sums over n + L - 1 samples and both channels:
    P_all e_j = least-squares projection of e_j (each channel on its own) on every s[i][c][n - tau], tau < L;  P_i e_j = on source i's alone
    e_spat = P_i e_j - s_i    e_interf = P_all e_j - P_i e_j    e_artif = e_j - P_all e_j
    SDR = 10 log10 |s_i|^2 / |e_j - s_i|^2                     ISR = 10 log10 |s_i|^2 / |e_spat|^2
    SIR = 10 log10 |s_i + e_spat|^2 / |e_interf|^2             SAR = 10 log10 |s_i + e_spat + e_interf|^2 / |e_artif|^2
A zero denominator gives +inf (one source: SIR = +inf).
"""
import itertools
import warnings

import numpy as np
import torch

from . import _eval

MAX_SOURCES = 8
# The dense Gram matrices of one chunk of files AND their transient copies stay under this: G is (J C L)^2 float64 per file (75 MB at
# J = 3, L = 512), and at the peak four of them are alive -- the gathered Toeplitz blocks, G itself, the diagonal blocks beside it and the
# LU factorisation's own copy.  4 GiB = 14 files per chunk at J = 3, L = 512.
GRAM_CAP_BYTES = 4 << 30
GRAM_COPIES = 4


def files_per_chunk(J, C, L, gram_cap_bytes=GRAM_CAP_BYTES):
    return max(1, int(gram_cap_bytes // (GRAM_COPIES * 8 * (J * C * L) ** 2)))


def check_images(referenceImages, estimatedImages, filterLength):
    """The argument rules of ``bss_eval_images``; no device needed.  Returns (s, e, batched): float32 arrays (batch, J, C, n).
    ValueError: unequal shapes, not (J, C, n) or (batch, J, C, n), C not 1 or 2, J > 8, filterLength not a whole number in [1, 4096],
    J * C * filterLength >= n + filterLength - 1 (more taps than samples: the Gram matrix is singular by construction), non-finite input."""
    s, e = np.asarray(referenceImages), np.asarray(estimatedImages)
    if s.shape != e.shape:
        raise ValueError('reference and estimated images must have the same shape, got %s and %s' % (s.shape, e.shape))
    batched = check_image_shape(s.shape, filterLength)
    if not batched:
        s, e = s[None], e[None]
    s, e = np.ascontiguousarray(s, dtype=np.float32), np.ascontiguousarray(e, dtype=np.float32)
    if not (np.isfinite(s).all() and np.isfinite(e).all()):
        raise ValueError('images are not finite everywhere')
    return s, e, batched


def check_image_shape(shape, filterLength):
    """The rules of ``check_images`` that need the shape alone.  Returns True for (batch, J, C, n), False for (J, C, n)."""
    shape = tuple(shape)
    if len(shape) not in (3, 4):
        raise ValueError('images have shape (J, C, n) or (batch, J, C, n), got %s' % (shape,))
    batched = len(shape) == 4
    B, J, C, n = shape if batched else (1,) + shape
    if B < 1 or J < 1 or n < 1:
        raise ValueError('images need at least one file, one source and one sample, got shape %s' % (shape,))
    if C not in (1, 2):
        raise ValueError('images have 1 or 2 channels (the layout is (..., J, C, n), not (nsrc, nsampl, nchan)), got C = %d' % C)
    if J > MAX_SOURCES:
        raise ValueError('at most %d sources per file, got %d' % (MAX_SOURCES, J))
    L = filterLength
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= L <= _eval.MAX_FILTER_LENGTH:
        raise ValueError('filterLength must be a whole number from 1 to %d, got %r' % (_eval.MAX_FILTER_LENGTH, L))
    if J * C * int(L) >= n + int(L) - 1:
        raise ValueError('J * C * filterLength = %d taps for %d samples: the Gram matrix is singular by construction'
                         % (J * C * int(L), n + int(L) - 1))
    return batched


def _solve(G, d):
    """G (m, k, k) float64 symmetric, d (m, k, r) -> (x, failed): one batched LU solve (``torch.linalg.solve_ex``); failed (m,) bool where
    the factorisation reports a zero pivot or the solution is not finite (x is zero there).
    Not Cholesky: on the ROCm build this was measured with (torch 2.10, float64, two 144 x 144 matrices of condition 200),
    ``torch.linalg.cholesky_ex`` returned a wrong factor in 5 of 6 repeats on identical input -- a non-zero info, or once info 0 with a
    residual of 0.14 -- while the LU solve was the same to the bit in all 6 (scripts/cholesky_repro.py reproduces it
    with torch alone, profiles/r22a_cholesky_repro.json)."""
    x, info = torch.linalg.solve_ex(G, d)
    failed = (info != 0) | ~torch.isfinite(x).all(dim=(1, 2))
    return torch.where(failed[:, None, None], torch.zeros_like(x), x), failed


def toeplitz_gram(Rss, L):
    """Rss (b, M, M, 2L - 1) lag correlations -> the dense Gram matrix (b, M L, M L), rows and columns ordered (signal, tau):
    G[(a, tau), (a', tau')] = Rss[a][a'][tau - tau' + L - 1]."""
    b, M = Rss.shape[:2]
    tau = torch.arange(L, device=Rss.device)
    idx = tau[:, None] - tau[None, :] + (L - 1)
    return Rss[:, :, :, idx].permute(0, 1, 3, 2, 4).reshape(b, M * L, M * L)


def projection_ranges(J, C, pairs, device):
    """(Q, 2) int32 [first_ref, num_refs] of the rows of ``projection_coefficients``: J C rows on every reference, then C rows per pair
    on the true source's own."""
    return torch.tensor([[0, J * C]] * (J * C) + [[i * C, C] for _, i in pairs for _ in range(C)], dtype=torch.int32, device=device)


def projection_coefficients(A, Et, J, L, pairs, workspace=None, stage=lambda name: (lambda: None)):
    """A, Et (b, J C, n) float32 device tensors (true images, estimates) -> (coef, failed): the filters (b, Q, J C, L) float64 of the
    Q = J C + len(pairs) C projections -- rows [0, J C): P_all of estimate channel (j, c''); then per pair (j, i) and channel c'': P_i of
    (j, c''), non-zero on source i's references only -- and failed (b,) bool where a file's solves did not succeed (its rows are zero)."""
    b, JC, n = A.shape
    C = JC // J
    CL, Np = C * L, len(pairs)
    done = stage('correlations')
    Rss = _eval.lag_correlations(A, A, L, workspace)
    Rse = _eval.lag_correlations(A, Et, L, workspace)
    done()
    done = stage('toeplitz')
    G = toeplitz_gram(Rss, L)
    d = Rse[..., L - 1:].permute(0, 1, 3, 2).reshape(b, JC * L, JC)           # d[(a, tau)][(j, c'')] = sum_n s_a[n - tau] e_jc''[n]
    G5 = G.view(b, J, CL, J, CL)
    Gi = torch.stack([G5[:, i, :, i, :] for i in range(J)], 1).reshape(b * J, CL, CL)
    di = d.view(b, J, CL, JC).reshape(b * J, CL, JC)
    done()
    done = stage('solves')
    x_all, failed_all = _solve(G, d)
    x_i, failed_i = _solve(Gi, di)
    failed = failed_all | failed_i.view(b, J).any(dim=1)
    done()
    done = stage('coefficients')
    coef = torch.zeros((b, JC + Np * C, JC, L), dtype=torch.float64, device=A.device)
    coef[:, :JC] = x_all.view(b, JC, L, JC).permute(0, 3, 1, 2)
    x6 = x_i.view(b, J, C, L, J, C)                                          # [file, i, c, tau, j, c'']
    rows = coef[:, JC:].view(b, Np, C, JC, L)
    for p, (j, i) in enumerate(pairs):
        rows[:, p, :, i * C:(i + 1) * C, :] = x6[:, i, :, :, j, :].permute(0, 3, 1, 2)
    coef[failed] = 0.0
    done()
    return coef, failed


def _aligned_chunk(X, f0, b):
    """Files [f0, f0 + b) of X (B, J, C, n) as a contiguous (b, J C, n) tensor whose address is a multiple of 16, as the kernels require:
    a slice of a contiguous tensor is a view at byte offset 4 f0 J C n, which for an odd n need not be -- such a chunk is copied."""
    B, J, C, n = X.shape
    chunk = X[f0:f0 + b].reshape(b, J * C, n).contiguous()
    return chunk.clone() if chunk.data_ptr() % 16 else chunk


def pair_energies(S, E, L, pairs, gram_cap_bytes=GRAM_CAP_BYTES, timings=None):
    """S, E (B, J, C, n) float32 DEVICE tensors; pairs: a list of (estimate j, true source i).  Returns (energies, status): a
    (B, len(pairs), 7) float64 host array of |s_i|^2, |P_i e_j - s_i|^2, |P_i e_j|^2, |P_all e_j - P_i e_j|^2, |P_all e_j|^2,
    |e_j - P_all e_j|^2, |e_j - s_i|^2 and a (B,) int array, 1 where a file's solves failed (its projections are then zero).
    Files go through in chunks of ``files_per_chunk`` whose dense Gram matrices, transient copies included, stay under ``gram_cap_bytes``;
    a file's figures do not depend on the chunking beyond the rounding of the batched solve.  timings: a dict that collects
    (stage name -> list of (start, end) device events) for scripts/bss_eval_bench.py."""
    B, J, C, n = S.shape
    M, JC = n + L - 1, J * C
    dev = S.device
    jidx = torch.tensor([p[0] for p in pairs], device=dev)
    iidx = torch.tensor([p[1] for p in pairs], device=dev)
    Np = len(pairs)
    ranges = projection_ranges(J, C, pairs, dev)
    per_chunk = files_per_chunk(J, C, L, gram_cap_bytes)
    out = np.zeros((B, Np, 7))
    status = np.zeros((B,), dtype=np.int64)

    def stage(name):
        if timings is None:
            return lambda: None
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        timings.setdefault(name, []).append(ev)
        ev[0].record()
        return ev[1].record

    workspace = None
    for f0 in range(0, B, per_chunk):
        b = min(per_chunk, B - f0)
        A, Et = _aligned_chunk(S, f0, b), _aligned_chunk(E, f0, b)
        need = _eval.workspace_bytes(JC, JC, n, L, b)
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        coef, failed = projection_coefficients(A, Et, J, L, pairs, workspace, stage)
        done = stage('projections')
        P = _eval.project(A, coef, ranges)
        done()
        done = stage('energies')
        s4 = torch.nn.functional.pad(A.double(), (0, L - 1)).view(b, J, C, M)[:, iidx]
        e4 = torch.nn.functional.pad(Et.double(), (0, L - 1)).view(b, J, C, M)[:, jidx]
        Pall = P[:, :JC].view(b, J, C, M)[:, jidx]
        Pi = P[:, JC:].view(b, Np, C, M)
        sq = lambda t: (t * t).sum(dim=(2, 3))
        en = torch.stack([sq(s4), sq(Pi - s4), sq(Pi), sq(Pall - Pi), sq(Pall), sq(e4 - Pall), sq(e4 - s4)], dim=2)
        done()
        out[f0:f0 + b] = en.cpu().numpy()
        status[f0:f0 + b] = failed.cpu().numpy()
        del P, Pall, Pi, s4, e4, coef
    return out, status


def _ratio_db(num, den):
    with np.errstate(divide='ignore', invalid='ignore'):
        r = 10.0 * np.log10(num / den)
    return np.where(den == 0, np.inf, r)


def criteria_from_energies(energies, status=None):
    """(..., 7) energies of ``pair_energies`` -> (sdr, isr, sir, sar) in dB; ISR, SIR and SAR are NaN where status is 1."""
    e = np.asarray(energies, dtype=np.float64)
    sdr, isr = _ratio_db(e[..., 0], e[..., 6]), _ratio_db(e[..., 0], e[..., 1])
    sir, sar = _ratio_db(e[..., 2], e[..., 3]), _ratio_db(e[..., 4], e[..., 5])
    if status is not None:
        lost = np.asarray(status).reshape((-1,) + (1,) * (e.ndim - 2)) != 0
        isr, sir, sar = (np.where(lost, np.nan, v) for v in (isr, sir, sar))
    return sdr, isr, sir, sar


def best_permutation(sir):
    """sir (J_est, J_true) -> perm (J,): estimate perm[i] goes to true source i, the assignment with the largest mean SIR (the first in
    itertools.permutations order on a tie); the identity if a SIR is NaN."""
    J = sir.shape[0]
    true = np.arange(J)
    if J == 1 or np.isnan(sir).any():
        return true
    best, best_mean = None, -np.inf
    for p in itertools.permutations(range(J)):
        m = np.mean(sir[list(p), true])
        if best is None or m > best_mean:
            best, best_mean = p, m
    return np.asarray(best)


def score_device(S, E, filterLength, computePermutation=True, allPairs=False, returnStatus=False, batched=True):
    """``bss_eval_images`` on float32 DEVICE tensors (B, J, C, n) that have passed the argument rules (the engines' ``score`` comes here
    with the waveforms where they lie)."""
    B, J = S.shape[:2]
    L = int(filterLength)
    every = computePermutation or allPairs
    pairs = [(j, i) for j in range(J) for i in range(J)] if every else [(i, i) for i in range(J)]
    energies, status = pair_energies(S, E, L, pairs)
    if status.any():
        warnings.warn('bss_eval_images: the projections of %d of %d files could not be solved (a silent or linearly dependent true source '
                      'image?): their ISR, SIR and SAR are NaN' % (int(status.sum()), B))
    if every:
        tables = criteria_from_energies(energies.reshape(B, J, J, 7), status)          # [file][estimate][true source]
        if allPairs:
            out = tables
        else:
            perm = np.stack([best_permutation(tables[2][f]) for f in range(B)])
            take = lambda t: np.take_along_axis(t, perm[:, None, :], axis=1)[:, 0, :]  # t[f][perm[f][i]][i]
            out = tuple(take(t) for t in tables) + (perm,)
    else:
        out = criteria_from_energies(energies, status) + (np.tile(np.arange(J), (B, 1)),)
    if not batched:
        out = tuple(v[0] for v in out)
    return out + (status if batched else status[0],) if returnStatus else out


def bss_eval_images(referenceImages, estimatedImages, filterLength=512, computePermutation=True, allPairs=False, device='cuda:0',
                    returnStatus=False):
    """SDR, ISR, SIR and SAR (dB) of BSS Eval 3.0 `bss_eval_images`, computed on the device.

    ``referenceImages`` / ``estimatedImages``: (J, C, n) or (batch, J, C, n) -- sources, channels (1 or 2), samples.  This is the ENGINE's
    layout (``GCCNMFEngine.separate`` returns (batch, S, 2, n)), NOT mir_eval's (nsrc, nsampl, nchan).  Scored as float32, which is what
    the kernels read.

    Returns ``(sdr, isr, sir, sar, perm)``, each (J,) or (batch, J), indexed by TRUE source: estimate ``perm[j]`` is true source j, the
    assignment with the largest mean SIR over all J x J pairs (J <= 8).  ``computePermutation=False`` scores estimate j against source j
    (perm is the identity).  ``allPairs=True`` returns the four tables (batch, J_est, J_true) -- or (J_est, J_true) -- instead, and no perm.
    ``returnStatus=True`` appends the per-file status: 1 where the LU solve of one of a file's Gram matrices failed
    (a silent or linearly dependent true image) -- ISR, SIR and SAR are then NaN, SDR is still the plain energy ratio -- for a silent true
    source itself that is 10 log10(0 / |e|^2) = -inf, finite for the file's other sources -- and one warning is issued per call.

    ValueError, before a device is looked for: unequal shapes, J > 8, C not 1 or 2, ``filterLength`` outside [1, 4096],
    J * C * filterLength >= n + filterLength - 1, non-finite input.  HipLibraryError without libgccnmf_eval.so or a device."""
    s, e, batched = check_images(referenceImages, estimatedImages, filterLength)
    _eval.require_device()
    dev = torch.device(device)
    with torch.cuda.device(dev):
        S, E = torch.from_numpy(s).to(dev), torch.from_numpy(e).to(dev)
        return score_device(S, E, filterLength, computePermutation, allPairs, returnStatus, batched)
