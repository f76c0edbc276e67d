"""Device-resident M-channel GCC-NMF for a batch of equally shaped microphone-array recordings.

GCC-NMF extends from a stereo pair to an array directly: the NMF runs on the magnitudes of all M channels side by side, the GCC-PHAT
functions of all P = M (M - 1) / 2 microphone pairs are summed (SRP-PHAT), and an atom is scored by the sum of its pairwise GCC-NMF
scores.  With the pairs STACKED along the bin axis (pair p owns rows p Fp .. p Fp + F - 1 of a matrix of Fs = (P - 1) Fp + F bins) both
sums are the stereo library calls at F = Fs; the two stages that know the channel count -- the per-pair coherence with the M-channel
magnitude matrix, and the masked reconstruction -- are libgccnmf_array.so (include/gccnmf_array.h, ``_array``).

Python here is plumbing only, as in ``engine``: every stage is one call into a library; the host computes the input-independent tables
(window, twiddles, steering cos / sin of the pair TDOAs, initial factors).
"""
import numpy as np
import torch

from . import _array, _array_em, _array_spatial, _hip
from .engine import (SPEED_OF_SOUND_IN_METRES_PER_SECOND, _on_device, num_frames, klnmf_initial_factors, fft_twiddles, steering_tables,
                     padded)

MAX_DIRECTIONS = 4096
RECONSTRUCTIONS = ('ratio', 'spatial')


def azimuthDirections(numDirections, startDeg=0.0, stopDeg=180.0):
    """(numDirections, 3) unit vectors (cos az, sin az, 0) for azimuths from startDeg to stopDeg inclusive: the candidate directions
    of a horizontal scan.  For a linear array along x, 0 .. 180 degrees is everything the array can tell apart."""
    az = np.deg2rad(np.linspace(float(startDeg), float(stopDeg), int(numDirections)))
    return np.stack([np.cos(az), np.sin(az), np.zeros_like(az)], axis=1)


def pairTDOAsFromGeometry(microphonePositions, directions, speedOfSound=SPEED_OF_SOUND_IN_METRES_PER_SECOND):
    """tau[p][d] = (r_b - r_a) . u_d / c in seconds, (P, D) float64, pairs (a, b), a < b, in lexicographic order.  r: microphone
    positions (M, 3) in metres; u_d: unit vectors from the array towards the candidate directions (far field).  This is the sign that
    goes with X = conj(fft) and C_ab = X_a conj(X_b): a source whose channel b is roll(s, +n) of channel a sits at tau = -n / sampleRate,
    as on the stereo path."""
    r = np.asarray(microphonePositions, np.float64)
    u = np.asarray(directions, np.float64)
    if r.ndim != 2 or r.shape[1] != 3 or not _array.MIN_CHANNELS <= r.shape[0] <= _array.MAX_CHANNELS:
        raise ValueError('microphonePositions must have shape (M, 3) with %d <= M <= %d, got %s'
                         % (_array.MIN_CHANNELS, _array.MAX_CHANNELS, r.shape))
    if u.ndim != 2 or u.shape[1] != 3:
        raise ValueError('directions must have shape (D, 3), got %s' % (u.shape,))
    if not (np.isfinite(r).all() and np.isfinite(u).all()):
        raise ValueError('microphonePositions and directions must be finite')
    if not np.allclose(np.sqrt((u ** 2).sum(axis=1)), 1.0, rtol=0, atol=1e-6):
        raise ValueError('directions must be unit vectors')
    if not (np.isfinite(speedOfSound) and speedOfSound > 0):
        raise ValueError('speedOfSound must be positive')
    return np.stack([(r[b] - r[a]).dot(u.T) / float(speedOfSound) for a, b in _array.pairs(r.shape[0])])


def array_steering_tables(frequenciesInHz, pairTDOAs, Fp, Dp):
    """cos / sin of 2 pi f tau[p][d], float64 then float32 as ``steering_tables`` does, stacked [2][P Fp][Dp]: pair p in rows
    p Fp .. p Fp + F - 1, zero elsewhere."""
    P = len(pairTDOAs)
    trig = np.zeros((2, P * Fp, Dp), np.float32)
    for p in range(P):
        trig[:, p * Fp:(p + 1) * Fp] = steering_tables(frequenciesInHz, pairTDOAs[p], Fp, Dp)
    return trig


def check_array_arguments(numChannels, pairTDOAs, microphonePositions, directions, speedOfSound, numTargets, windowSize):
    """The arguments of GCCNMFArrayEngine that need no device -> (M, pairTDOAs (P, D) float64, numTargets); ValueError otherwise."""
    M = numChannels
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or not _array.MIN_CHANNELS <= M <= _array.MAX_CHANNELS:
        raise ValueError('numChannels must be an integer in %d..%d, got %r' % (_array.MIN_CHANNELS, _array.MAX_CHANNELS, M))
    M = int(M)
    S = numTargets
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= S <= _array.MAX_TARGETS:
        raise ValueError('numTargets must be an integer in 1..%d, got %r' % (_array.MAX_TARGETS, S))
    n_fft = windowSize
    if isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or not 64 <= n_fft <= 4096 or n_fft & (n_fft - 1):
        raise ValueError('windowSize must be a power of two in 64..4096, got %r' % (n_fft,))
    if pairTDOAs is not None:
        if microphonePositions is not None or directions is not None:
            raise ValueError('give either pairTDOAs or microphonePositions and directions, not both')
        tau = np.array(pairTDOAs, dtype=np.float64)
    else:
        if microphonePositions is None or directions is None:
            raise ValueError('give pairTDOAs, or microphonePositions and directions')
        r = np.asarray(microphonePositions, np.float64)
        if r.ndim != 2 or r.shape != (M, 3):
            raise ValueError('microphonePositions must have shape (%d, 3), got %s' % (M, r.shape))
        tau = pairTDOAsFromGeometry(r, directions, speedOfSound)
    P = _array.num_pairs(M)
    if tau.ndim != 2 or tau.shape[0] != P:
        raise ValueError('pairTDOAs must have shape (%d, D) for %d channels, got %s' % (P, M, tau.shape))
    if not 3 <= tau.shape[1] <= MAX_DIRECTIONS:
        raise ValueError('between 3 and %d candidate directions are needed, got %d' % (MAX_DIRECTIONS, tau.shape[1]))
    if not np.isfinite(tau).all():
        raise ValueError('pairTDOAs must be finite')
    return M, tau, int(S)


class GCCNMFArrayEngine(object):
    """All buffers of one batch shape of M-channel recordings, allocated once; ``separate()`` runs the full path on the device.

    Either ``pairTDOAs`` -- a (P, D) float64 table of the TDOA in seconds of every microphone pair (a, b), a < b, in lexicographic
    order, for each of D candidate directions -- or ``microphonePositions`` (M, 3) and unit ``directions`` (D, 3), from which the table
    is tau[p][d] = (r_b - r_a) . u_d / speedOfSound (``pairTDOAsFromGeometry``; ``azimuthDirections`` makes a horizontal scan).

    The candidate directions are an OPEN one-dimensional sequence: a direction is a peak when its mean SRP-PHAT value is larger than
    that of both neighbours in the sequence, so -- as on the stereo path -- the two end points never qualify as peaks.

    Stages are named as in ``GCCNMFEngine``: upload, stft, klnmf, localize, masks, reconstruct, istft, run, separate.  At most 8 targets.
    ``reconstruction='ratio'`` (the default) is the ratio mask: the targets of a channel add up to that channel's mixture, and a mask
    weights each channel by a real number.  ``reconstruction='spatial'`` runs the M x M spatial (multichannel Wiener) filter behind it
    (libgccnmf_array_spatial.so, include/gccnmf_array_spatial.h): a spatial covariance per target and bin from the ratio estimates, then
    S'_i = v_i R_i (sum_j v_j R_j)^-1 X, which combines the channels; ``get_cov()`` returns the covariances.
    ``spatialIterations=n`` (0 to 255, default 0; 'spatial' only) runs n iterations of the local Gaussian model EM between the two
    (libgccnmf_array_em.so, include/gccnmf_array_em.h): a full-rank M x M covariance per target and bin and the powers are re-estimated
    against each other, and the filter runs on the refined ones; ``get_cov()`` then returns the refined covariances.  With M = 2 and
    ``pairTDOAs = tdoasInSeconds[None]`` every buffer holds the bits of ``GCCNMFEngine(reconstruction=..., spatialIterations=..., nmf_groups=1)``
    in the same mode.

    ``separate(x)``: (batch, M, n_samples) float32 -> (batch, S, M, hop * (T - 1)) float32."""

    def __init__(self, n_samples, numChannels=2, pairTDOAs=None, microphonePositions=None, directions=None,
                 speedOfSound=SPEED_OF_SOUND_IN_METRES_PER_SECOND, sampleRate=16000, windowSize=1024, hopSize=256, numTargets=3,
                 dictionarySize=128, numIterations=100, sparsityAlpha=0, epsilon=1e-16, seedValue=0, batch=1, windowFunction=np.hanning,
                 device='cuda:0', klnmf_flags=0, reconstruction='ratio', spatialIterations=0):
        if reconstruction not in RECONSTRUCTIONS:
            raise ValueError("reconstruction must be 'ratio' or 'spatial', got %r" % (reconstruction,))
        self.reconstruction = reconstruction
        self.spatialIterations = _hip.check_spatial_iterations(spatialIterations, reconstruction)
        self.M, self.pairTDOAs, S = check_array_arguments(numChannels, pairTDOAs, microphonePositions, directions, speedOfSound,
                                                          numTargets, windowSize)
        self.P = _array.num_pairs(self.M)
        if int(batch) < 1 or int(dictionarySize) < 1 or int(hopSize) < 1:
            raise ValueError('batch, dictionarySize and hopSize must be positive')
        self.n_samples, self.sampleRate = int(n_samples), sampleRate
        self.n_fft, self.hop = int(windowSize), int(hopSize)
        F = self.n_fft // 2 + 1
        T = num_frames(self.n_samples, self.n_fft, self.hop)
        if T < 2:
            raise ValueError('Buffer is too short (n=%d) for frame_length=%d' % (n_samples, self.n_fft))
        if not torch.cuda.is_available():
            raise _hip.HipLibraryError('no ROCm device visible: the GCC-NMF HIP path has no CPU fallback')
        self.lib = _hip.lib()
        _array.lib()
        if reconstruction == 'spatial':
            _array_spatial.lib()
        if self.spatialIterations:
            _array_em.lib()
        self.device = torch.device(device)
        self.iters, self.alpha, self.eps, self.seed = int(numIterations), float(sparsityAlpha), float(epsilon), seedValue
        self.batch = B = int(batch)
        self.klnmf_flags = klnmf_flags
        M, P = self.M, self.P
        self.F, self.T, self.K, self.S, self.D = F, T, int(dictionarySize), S, self.pairTDOAs.shape[1]
        K, D = self.K, self.D
        self.N = M * T
        rup = lambda a, b: -(-a // b) * b
        self.Fp, self.Kp, self.Tp, self.Np, self.Dp = rup(F, 16), rup(K, 64), rup(T, 64), rup(M * T, 64), rup(D, 64)
        self.Fs = (P - 1) * self.Fp + F                               # stacked bins; round_up(Fs, 16) = P Fp
        self.nsig_pitch = rup(S * M, 2)                               # the iSTFT transforms signals in pairs: one spare zero slot if S M is odd
        self.L = self.hop * (T - 1)
        self.nstft = -(-(B * M) // 2)                                 # the STFT takes the batch * M signals as consecutive pairs
        Fp, Kp, Tp, Np, Dp = self.Fp, self.Kp, self.Tp, self.Np, self.Dp
        dev, f32 = self.device, torch.float32

        with torch.cuda.device(dev):
            self.window = torch.from_numpy(np.asarray(windowFunction(self.n_fft), np.float64).astype(np.float32)).to(dev)
            self.twiddle = torch.from_numpy(fft_twiddles(self.n_fft)).to(dev)
            self.frequenciesInHz = np.linspace(0, sampleRate / 2.0, F)
            self.trig = torch.from_numpy(array_steering_tables(self.frequenciesInHz, self.pairTDOAs, Fp, Dp)).to(dev)
            W0, H0 = klnmf_initial_factors(F, self.N, K, self.eps, seedValue)
            self.W0 = padded(W0, (Fp, Kp), dev)
            self.H0 = padded(H0, (Kp, Np), dev)

            z = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
            # batch * M signals, one spare zero signal (and spectrogram slot) when that number is odd
            self._x = z(2 * self.nstft, self.n_samples)
            self.x = self._x[:B * M].view(B, M, self.n_samples)
            self._X = z(2 * self.nstft, Fp, Tp, 2)
            self.X = self._X[:B * M].view(B, M, Fp, Tp, 2)
            self.V = z(B, Fp, Np)
            self.CC = z(B, 2, P * Fp, Tp)
            self.W = z(B, Fp, Kp)
            self.H = z(B, Kp, Np)
            self.Ws = z(B, P * Fp, Kp)
            self.ws_nmf = z(_hip.klnmf_divergence_workspace_floats(F, self.N, K, B))
            self.ang = z(B, Dp, Tp)
            self.mean_ang = torch.zeros((B, Dp), dtype=torch.float64, device=dev)
            self.tdoa_idx = torch.zeros((B, S), dtype=torch.int32, device=dev)
            self.status = torch.zeros((B,), dtype=torch.int32, device=dev)
            need = self.lib.gccnmf_scores_workspace_floats(self.Fs, T, S, B)
            if need < 0:
                raise _hip.HipLibraryError('gccnmf_scores_workspace_floats rejected the stacked shape')
            self.ws_scores = z(need)
            self.scores = z(B, Kp, S * Tp)
            self.argmax = torch.zeros((B, Kp, Tp), dtype=torch.uint8, device=dev)
            self.spec = z(B, self.nsig_pitch, Fp, Tp, 2)              # (the spare slot stays zero: the reconstruction does not touch it)
            # spatial mode: R~ of every (file, target, bin), M M floats a row (include/gccnmf_array_spatial.h)
            # with the EM refinement the same rows open its workspace, and the powers v [batch][S][Fp][Tp] follow them (include/gccnmf_array_em.h)
            self.cov = self.ws_em = self.powers = None
            if self.spatialIterations:
                self.ws_em = z(_array_em.workspace_floats(M, F, T, S, B))
                self.cov = self.ws_em[:B * S * Fp * M * M].view(B, S, Fp, M * M)
                self.powers = self.ws_em[B * S * Fp * M * M:].view(B, S, Fp, Tp)
            elif reconstruction == 'spatial':
                self.cov = z(_array_spatial.workspace_floats(M, F, S, B)).view(B, S, Fp, M * M)
            self.frames = None
            # the stereo engine's rule: the fused inverse transform + overlap-add where the library has one and the launch is large enough
            self.fused_istft = (self.n_fft + 3 * self.hop <= 2048 and self.hop <= self.n_fft
                                and B * (self.nsig_pitch // 2) * -(-T // 32) >= 256)
            self._y = z(B, self.nsig_pitch, self.L)                   # waveform (i, c) of a file in slot i M + c: get_y()

    # ---- stages (each asynchronous on the current torch stream) ---------------------------------
    @_on_device
    def upload(self, samples):
        self.x.copy_(torch.from_numpy(np.ascontiguousarray(self._checked_samples(samples))))

    def _checked_samples(self, samples):
        x = np.asarray(samples, dtype=np.float32)
        if x.ndim == 2:
            x = x[None]
        if x.shape != (self.batch, self.M, self.n_samples):
            raise ValueError('expected samples of shape %s, got %s' % ((self.batch, self.M, self.n_samples), x.shape))
        if not np.isfinite(x).all():
            raise ValueError('Audio buffer is not finite everywhere')
        return x

    @_on_device
    def stft(self):
        """X of all batch * M signals (as consecutive stereo pairs, without the pair's own V and coherence), then the array features."""
        _hip.stft_stereo(self._x, self.n_samples, self.n_fft, self.hop, self.T, self.nstft, self.window, self.twiddle, self._X, None, None)
        _array.features(self.X, self.M, self.F, self.T, self.batch, self.V, self.CC)

    @_on_device
    def klnmf(self):
        self.W.copy_(self.W0.unsqueeze(0).expand_as(self.W))
        self.H.copy_(self.H0.unsqueeze(0).expand_as(self.H))
        _hip.klnmf(self.V, self.W, self.H, self.ws_nmf, self.F, self.N, self.K, self.batch, self.iters, self.alpha, self.eps,
                   flags=self.klnmf_flags)

    @_on_device
    def localize(self):
        _hip.angular_spectrogram(self.CC, self.trig, self.Fs, self.T, self.D, self.batch, self.ang, self.mean_ang)
        _hip.pick_tdoa_peaks(self.mean_ang, self.D, self.Dp, self.S, self.batch, self.tdoa_idx, self.status)

    @_on_device
    def masks(self):
        Fp = self.Fp
        for p in range(self.P):                      # the file's W block under every pair's rows (a copy: the GEMM reads one matrix)
            self.Ws[:, p * Fp:(p + 1) * Fp].copy_(self.W)
        _hip.target_scores_masks(self.CC, self.trig, self.tdoa_idx, self.Ws, self.Fs, self.T, self.K, self.D, self.S, self.batch,
                                 self.ws_scores, self.scores, self.argmax)

    @_on_device
    def reconstruct(self):
        _array.reconstruct(self.W, self.H, self.argmax, None, self.X, self.M, self.F, self.T, self.K, self.S, self.batch, self.nsig_pitch,
                           self.spec)
        if self.spatialIterations:
            _array_em.em(self.X, self.M, self.F, self.T, self.S, self.batch, self.nsig_pitch, self.spatialIterations, self.ws_em, self.spec)
        elif self.reconstruction == 'spatial':
            _array_spatial.spatial(self.X, self.M, self.F, self.T, self.S, self.batch, self.nsig_pitch, self.cov, self.spec)

    @_on_device
    def istft(self, keep_frames=False):
        gain = np.float32(self.hop / float(self.n_fft) * 2)
        frames = None
        if keep_frames or not self.fused_istft:
            if self.frames is None:
                self.frames = torch.zeros((self.batch, self.nsig_pitch, self.T, self.n_fft), dtype=torch.float32, device=self.device)
            frames = self.frames
        _hip.istft_ola(self.spec, self.nsig_pitch, self.n_fft, self.hop, self.T, self.batch, self.window, self.twiddle, gain, True, frames,
                       self._y)

    @_on_device
    def run(self, stft=True):
        """samples already in ``self.x`` -> separated waveforms on the device (asynchronous)."""
        if stft:
            self.stft()
        self.klnmf()
        self.localize()
        self.masks()
        self.reconstruct()
        self.istft()

    @_on_device
    def separate(self, samples):
        """(batch, M, n_samples) float32 host samples -> (batch, S, M, hop * (T - 1)) float32 host waveforms."""
        self.upload(samples)
        self.run()
        y = self.get_y()
        self.check_status()
        return y

    # ---- results ---------------------------------------------------------------------------------
    @_on_device
    def check_status(self):
        torch.cuda.current_stream(self.device).synchronize()
        st = _hip.klnmf_chain_status(self.ws_nmf, self.F, self.N, self.K, self.batch)
        if st:
            raise _hip.HipLibraryError('the chained KL-NMF launch did not hand over cleanly (status %d): W and H of this batch are NaN.  '
                                       'GCCNMF_TUNE="21=0" runs the plain launches.' % st)
        st = self.status.cpu().numpy()
        if st.any():
            raise ValueError('fewer than %d angular-spectrum peaks in file(s) %s' % (self.S, np.nonzero(st)[0].tolist()))

    def get_y(self):
        return self._y[:, :self.S * self.M].reshape(self.batch, self.S, self.M, self.L).cpu().numpy()

    def get_X(self):
        return torch.view_as_complex(self.X)[:, :, :self.F, :self.T].cpu().numpy()

    def get_V(self):
        return self.V[:, :self.F, :self.N].cpu().numpy()

    def get_C(self):
        """(batch, P, F, T) complex64: the PHAT coherence of every pair."""
        c = self.CC.view(self.batch, 2, self.P, self.Fp, self.Tp)[:, :, :, :self.F, :self.T].cpu().numpy()
        return (c[:, 0] + 1j * c[:, 1]).astype(np.complex64)

    def get_WH(self):
        return self.W[:, :self.F, :self.K].cpu().numpy(), self.H[:, :self.K, :self.N].cpu().numpy()

    def get_angular(self):
        return self.ang[:, :self.D, :self.T].cpu().numpy(), self.mean_ang[:, :self.D].cpu().numpy()

    def get_tdoa_indexes(self):
        """(batch, S) int32: the indexes of the chosen directions in the candidate sequence, ascending per file."""
        return self.tdoa_idx.cpu().numpy()

    def get_scores(self):
        """(batch, S, K, T)"""
        s = self.scores.view(self.batch, self.Kp, self.S, self.Tp)[:, :self.K, :, :self.T]
        return s.permute(0, 2, 1, 3).contiguous().cpu().numpy()

    def get_argmax(self):
        return self.argmax[:, :self.K, :self.T].cpu().numpy()

    def get_cov(self):
        """(batch, S, F, M, M) complex64: the loaded spatial covariance R~ of every target and bin, the full Hermitian matrix
        (spatial mode only; after ``spatialIterations`` EM iterations, the refined one)."""
        if self.cov is None:
            raise ValueError("get_cov() needs reconstruction='spatial'")
        M = self.M
        rows = self.cov[:, :, :self.F].cpu().numpy()
        R = np.zeros((self.batch, self.S, self.F, M, M), np.complex64)
        for a in range(M):                                    # a row: the M diagonal entries, then (Re, Im) of the pairs in the library's order
            R[..., a, a] = rows[..., a]
        for k, (a, b) in enumerate(_array.pairs(M)):
            R[..., a, b] = rows[..., M + 2 * k] + 1j * rows[..., M + 2 * k + 1]
            R[..., b, a] = rows[..., M + 2 * k] - 1j * rows[..., M + 2 * k + 1]
        return R

    def get_spec(self):
        """(batch, S, M, F, T) complex64"""
        s = torch.view_as_complex(self.spec)[:, :self.S * self.M, :self.F, :self.T]
        return s.reshape(self.batch, self.S, self.M, self.F, self.T).cpu().numpy()
