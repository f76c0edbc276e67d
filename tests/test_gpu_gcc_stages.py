"""-m gpu: the stages after KL-NMF (csrc/gcc.hip) called directly through the C ABI, off the n_fft = 1024 path.

Inputs are built on the host (random unit-modulus coherence, W, H >= 0, given TDOA indexes), so nothing upstream drifts, and every
result is compared with a float64 NumPy evaluation of the SAME float32 inputs under the worst-case bounds of tests/gcc_checks.py.  The
Nyquist row of W and C and the last reduction index of each GEMM are 100x larger than the rest, so that a kernel that drops or misplaces
them is far outside the bound.  Output buffers and workspaces are NaN-filled before every call: every logical element must be written,
the padding the geometry promises (and the next stage reads) must be zero, and a second call over a workspace of other garbage must give
the same bits.

The cases are chosen by the launch rules of gcc.hip with tuning keys 2 (0 by size, 1 throughput tile, 2 small ring tile) and 3 (1 LDS-DMA,
0 register-staged); CELLS (tests/gcc_stage_inputs.py, with the input builders) names the kernel each stage of a case reaches.
"""
import numpy as np
import pytest

import gcc_checks as C
from gcc_stage_inputs import CELLS, CELL_IDS, cell_seed, geometry, host_file, tuning, upload
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ERR_ARG = 1
GARBAGE = 1e30


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr()


def nan_like(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def run_stages(lib, files, F, T, K, D, S, trig):
    """Every gcc.hip stage on a batch: angular spectrogram + mean, peaks, scores + arg-max (given TDOA indexes), reconstruction with the
    device arg-max and with soft masks.  Outputs and workspaces NaN-filled before each call; the scores and reconstruction run a second
    time over a workspace of other garbage, which must give the same bits.  -> dict of host arrays."""
    g = geometry(F, T, K, D)
    B = len(files)
    dv = upload(files, g, S)
    r = {'g': g}
    s = stream()

    ang, mean = nan_like((B, g.Dp, g.Tp)), nan_like((B, g.Dp), torch.float64)
    assert lib.gccnmf_angular_spectrogram(ptr(dv['CC']), ptr(trig), F, T, D, B, ptr(ang), ptr(mean), s) == 0
    idx, status = torch.full((B, S), -7, dtype=torch.int32, device='cuda'), torch.full((B,), -7, dtype=torch.int32, device='cuda')
    if D >= 3:
        assert lib.gccnmf_pick_tdoa_peaks(ptr(mean), D, g.Dp, S, B, ptr(idx), ptr(status), s) == 0

    nws = lib.gccnmf_scores_workspace_floats(F, T, S, B)
    assert nws == B * g.Fp * S * g.Tp
    runs = []
    for fill in (float('nan'), GARBAGE):
        ws = torch.full((nws,), fill, dtype=torch.float32, device='cuda')
        scores = nan_like((B, g.Kp, S * g.Tp))
        am = torch.full((B, g.Kp, g.Tp), 0xAB, dtype=torch.uint8, device='cuda')
        assert lib.gccnmf_target_scores_masks(ptr(dv['CC']), ptr(trig), ptr(dv['tdoa']), ptr(dv['W']), F, T, K, D, S, B, ptr(ws),
                                              ptr(scores), ptr(am), s) == 0
        runs.append((ws, scores, am))
    dev_argmax = runs[0][2]
    torch.cuda.synchronize()
    r['P'] = runs[0][0].view(B, g.Fp, S, g.Tp).cpu().numpy()
    r['scores'] = runs[0][1].view(B, g.Kp, S, g.Tp).cpu().numpy()
    r['argmax'] = dev_argmax.cpu().numpy()
    assert np.array_equal(runs[1][1].cpu().numpy(), runs[0][1].cpu().numpy(), equal_nan=True), 'scores depend on the workspace'
    assert np.array_equal(runs[1][2].cpu().numpy(), r['argmax']), 'arg-max depends on the workspace'

    nwr = lib.gccnmf_reconstruct_workspace_floats(T, K, S, B)
    assert nwr == B * g.Kp * 2 * S * g.Tp
    for form in ('argmax', 'masks'):
        runs = []
        for fill in (float('nan'), GARBAGE):
            ws = torch.full((nwr,), fill, dtype=torch.float32, device='cuda')
            spec = nan_like((B, 2 * S, g.Fp, g.Tp, 2))
            am, m = (ptr(dev_argmax), 0) if form == 'argmax' else (0, ptr(dv['masks']))
            assert lib.gccnmf_reconstruct(ptr(dv['W']), ptr(dv['H']), am, m, ptr(dv['X']), ptr(dv['V']), F, T, K, S, B, ptr(ws),
                                          ptr(spec), s) == 0
            runs.append((ws, spec))
        torch.cuda.synchronize()
        r['Hm_' + form] = runs[0][0].view(B, g.Kp, S, 2, g.Tp).cpu().numpy()
        sp = runs[0][1].cpu().numpy()
        r['spec_' + form] = (sp[..., 0] + 1j * sp[..., 1]).reshape(B, S, 2, g.Fp, g.Tp)
        assert np.array_equal(runs[1][1].cpu().numpy(), sp, equal_nan=True), 'reconstruction (%s) depends on the workspace' % form
    r['ang'] = ang.cpu().numpy()
    r['mean'] = mean.cpu().numpy()
    r['idx'] = idx.cpu().numpy()
    r['status'] = status.cpu().numpy()
    return r


def check_file(r, b, f, F, T, K, D, S, freqs, tdoas):
    """File b of run_stages() against float64 evaluations of its own float32 inputs."""
    g = r['g']
    Cc = f['C'].astype(np.complex128)
    E = np.exp(np.outer(freqs, -(2j * np.pi) * tdoas))                                   # (F, D), as the oracle's steering table
    what = lambda name: '%s (file %d)' % (name, b)

    # angular spectrogram A = Re(E^T C): the oracle's own expression; reduction = 2F real terms
    ang = r['ang'][b, :D, :T]
    absA = np.dot(np.abs(E.real).T, np.abs(Cc.real)) + np.dot(np.abs(E.imag).T, np.abs(Cc.imag))
    C.check_gemm_like(ang, O.getAngularSpectrogram(Cc, freqs, 1.0, D), absA, 2 * F, what=what('angular spectrogram'))
    C.check_mean(r['mean'][b, :D], ang, what=what('mean_ang'))
    if D >= 3:
        C.check_peaks(r['idx'][b], r['status'][b], r['mean'][b, :D], S, what=what('peaks'))
        if r['status'][b] == 0:                # distinct random heights: exactly the oracle's localisation
            assert r['idx'][b].tolist() == O.estimateTargetTDOAIndexesFromAngularSpectrum(r['mean'][b, :D], 1.0, D, S)

    # steering products P_i = Re(C e_i) (workspace of the scores call) and scores G_i = W^T P_i
    W64, H64 = f['W'].astype(np.float64), f['H'].astype(np.float64)
    P = r['P'][b]
    for i, tau in enumerate(f['tdoa']):
        e = E[:, tau][:, None]
        Pabs = np.abs(Cc.real) * np.abs(e.real) + np.abs(Cc.imag) * np.abs(e.imag)
        C.check_gemm_like(P[:F, i, :T], (Cc * e).real, Pabs, 1, what=what('steering product, target %d' % i))
        C.check_gemm_like(r['scores'][b, :K, i, :T], np.dot(W64.T, (Cc * e).real), np.dot(np.abs(W64).T, Pabs), F,
                          what=what('scores, target %d' % i))
    C.check_zero(P[F:], what=what('steering product, padded bins'))
    C.check_zero(P[:, :, T:], what=what('steering product, padded frames'))
    C.check_zero(r['scores'][b, :K, :, T:], what=what('scores, padded frames'))

    # arg-max: numpy.nanargmax of the device's own scores, exactly; padding 0
    am = r['argmax'][b]
    C.check_argmax(am[:K, :T], np.transpose(r['scores'][b, :K, :, :T], (1, 0, 2)), what=what('arg-max'))
    C.check_zero(am[K:], what=what('arg-max, padded atoms'))
    C.check_zero(am[:, T:], what=what('arg-max, padded frames'))

    # reconstruction S[i,c] = (W (H_c o M_i)) X_c / |X_c| with one-hot masks of that arg-max, and with the soft masks
    phase = np.exp(1j * np.angle(f['X'].astype(np.complex128)))
    onehot = np.stack([(am[:K, :T] == i) for i in range(S)]).astype(np.float32)
    for form, M in (('argmax', onehot), ('masks', f['masks'])):
        Hm = r['Hm_' + form][b]
        spec = r['spec_' + form][b]
        for i in range(S):
            for c in range(2):
                Hc = f['H'][:, c * T:(c + 1) * T]
                assert np.array_equal(Hm[:K, i, c, :T], Hc * M[i]), what('masked H (%s), target %d channel %d' % (form, i, c))
                ref = np.dot(W64, Hc.astype(np.float64) * M[i]) * phase[c]
                absprod = np.dot(np.abs(W64), np.abs(Hc.astype(np.float64) * M[i]))
                C.check_gemm_like(spec[i, c, :F, :T], ref, absprod, K, what=what('reconstruction (%s), target %d channel %d' % (form, i, c)))
        C.check_zero(Hm[K:], what=what('masked H (%s), padded atoms' % form))
        C.check_zero(Hm[..., T:], what=what('masked H (%s), padded frames' % form))


@pytest.mark.parametrize('F,D,S,K,T,batch,key2,key3', list(CELLS), ids=CELL_IDS)
def test_gcc_stages_against_float64(lib, F, D, S, K, T, batch, key2, key3):
    from gcc_nmf_amd.engine import steering_tables
    g = geometry(F, T, K, D)
    freqs = O.getFrequenciesInHz(16000, F)
    tdoas = O.getTDOAsInSeconds(1.0, D)
    trig = torch.from_numpy(steering_tables(freqs, tdoas, g.Fp, g.Dp)).cuda()
    files = [host_file(F, T, K, D, S, cell_seed(F, K, b)) for b in range(batch)]
    with tuning(lib, key2, key3):
        r = run_stages(lib, files, F, T, K, D, S, trig)
        alone = [run_stages(lib, [files[b]], F, T, K, D, S, trig) for b in sorted({0, batch - 1})] if batch > 1 else []
    for b in range(batch):
        check_file(r, b, files[b], F, T, K, D, S, freqs, tdoas)
    # a file's result does not depend on the batch it rides in (same kernels: forced tile policy; key 2 = 0 may pick another kernel for
    # one file, whose result must then only meet the bounds)
    for b, a in zip(sorted({0, batch - 1}), alone):
        check_file(a, 0, files[b], F, T, K, D, S, freqs, tdoas)
        if key2 != 0:
            for name in ('ang', 'mean', 'idx', 'scores', 'argmax', 'spec_argmax', 'spec_masks'):
                assert np.array_equal(r[name][b], a[name][0], equal_nan=True), (name, b)


def test_peaks_ties_plateaus_nan_edges(lib):
    """gccnmf_pick_tdoa_peaks on built spectra: exact ties at the S boundary (the larger index is kept), ties across
    lanes of the 64-lane reduction, plateaus, NaN, peaks at 1 and D - 2, D = 3 / 4096, fewer than S peaks (status 1, -1 slots) -- and
    random spectra with distinct heights, exactly the oracle's localisation."""
    rng = np.random.RandomState(5)

    def built(D):
        out = []
        if D == 3:
            out += [(np.array([0.0, 1.0, 0.0]), 1), (np.array([0.0, 1.0, 0.0]), 2), (np.array([1.0, 1.0, 0.0]), 1),
                    (np.array([0.0, np.nan, 0.0]), 1)]
            return out
        v = np.zeros(D)
        v[[1, D - 2]] = 1.0                                     # peaks at both ends of the interior, tied
        out += [(v, 1), (v, 2), (v, 3)]
        if D >= 12:
            w = np.zeros(D)
            w[[2, 5, 8]] = 1.0                                  # three equal peaks, two kept: 5 and 8
            w[10] = 2.0
            out += [(w, 3), (w, 2), (w, 1)]
            p = np.zeros(D)
            p[3] = p[4] = 3.0                                   # plateau: not a strict maximum
            p[7] = np.nan                                       # NaN: neither a peak nor greater than a neighbour
            p[6] = p[9] = 1.0
            out += [(p, 1), (p, 3)]
        if D >= 200:
            t = np.zeros(D)
            t[[3, 67, 131, 195, 36, 100, 164]] = 5.0            # equal heights in one lane (64 apart) and across lanes
            out += [(t, 3), (t, 5), (t, 1)]
        return out

    for D in (3, 4, 33, 64, 128, 129, 200, 4096):
        cases = built(D) + [(rng.standard_normal(D), S) for S in (1, 2, 3, 4, 7) for _ in range(3)]
        Dp = -(-D // 64) * 64
        for S in sorted({S for _, S in cases}):
            spectra = [v for v, s in cases if s == S]
            m = np.full((len(spectra), Dp), GARBAGE)           # padding beyond D must not be read
            for b, v in enumerate(spectra):
                m[b, :D] = v
            dm = torch.from_numpy(m).cuda()
            idx = torch.full((len(spectra), S), -7, dtype=torch.int32, device='cuda')
            st = torch.full((len(spectra),), -7, dtype=torch.int32, device='cuda')
            assert lib.gccnmf_pick_tdoa_peaks(ptr(dm), D, Dp, S, len(spectra), ptr(idx), ptr(st), stream()) == 0
            torch.cuda.synchronize()
            idx, st = idx.cpu().numpy(), st.cpu().numpy()
            for b, v in enumerate(spectra):
                C.check_peaks(idx[b], st[b], v, S, what='D = %d, S = %d, spectrum %d' % (D, S, b))
                if st[b] == 0 and not np.isnan(v).any():
                    assert idx[b].tolist() == O.estimateTargetTDOAIndexesFromAngularSpectrum(v, 1.0, D, S), (D, S, b)
    # the issue's example: the oracle and the device keep [10, 20]
    v = np.zeros(30)
    v[5], v[10], v[20] = 1.0, 1.0, 2.0
    dm = torch.from_numpy(np.concatenate([v, np.zeros(34)])).cuda()
    idx, st = torch.zeros(2, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    assert lib.gccnmf_pick_tdoa_peaks(ptr(dm), 30, 64, 2, 1, ptr(idx), ptr(st), stream()) == 0
    assert idx.cpu().numpy().tolist() == [10, 20] == O.estimateTargetTDOAIndexesFromAngularSpectrum(v, 1.0, 30, 2)
    # host-rejected arguments
    for D, Dp, S in ((4097, 4160, 1), (33, 64, 0), (2, 64, 1), (65, 64, 1)):
        assert lib.gccnmf_pick_tdoa_peaks(ptr(dm), D, Dp, S, 1, ptr(idx), ptr(st), stream()) == ERR_ARG, (D, Dp, S)


@pytest.mark.parametrize('S', [1, 2, 3, 7])
@pytest.mark.parametrize('T', [1, 2, 3, 5, 63, 64, 65, 130])
def test_argmax_ties_nan_tail_frames(lib, T, S):
    """gccnmf_argmax_targets = numpy.nanargmax exactly (first target on ties, NaN ignored), with ties and NaN in the last frames (T % 4
    != 0 puts them inside a thread's four-frame group); padded frames and atoms 0, although the last target's padding holds GARBAGE."""
    from gcc_nmf_amd.engine import Geometry
    K, B = 70, 2
    g = Geometry(2, T, K)
    rng = np.random.RandomState(T * 10 + S)
    sc = rng.randint(0, 3, (B, S, K, T)).astype(np.float32)       # three levels: ties everywhere
    if S > 1:
        nan = rng.rand(B, S, K, T) < 0.2
        nan[:, -1] = False                                         # never a column of NaN only (nanargmax raises there)
        sc[nan] = np.nan
        for t in range(max(0, T - 3), T):                          # the tail frames: a full tie, NaN ahead of a tie, NaN then the max
            sc[:, :, 0, t] = 1.0
            sc[:, 0, 1, t] = np.nan
            sc[:, 1:, 1, t] = 2.0
            sc[:, 0, 2, t] = np.nan
            sc[:, S - 1, 2, t] = 9.0
    img = np.zeros((B, g.Kp, S, g.Tp), np.float32)
    img[:, :, -1] = GARBAGE                                        # padding: read into a frame, it would win for the last target
    img[:, :K, :, :T] = np.transpose(sc, (0, 2, 1, 3))
    ds = torch.from_numpy(img).cuda()
    am = torch.full((B, g.Kp, g.Tp), 0xAB, dtype=torch.uint8, device='cuda')
    assert lib.gccnmf_argmax_targets(ptr(ds), K, T, S, B, ptr(am), stream()) == 0
    torch.cuda.synchronize()
    am = am.cpu().numpy()
    for b in range(B):
        C.check_argmax(am[b, :K, :T], sc[b], what='arg-max (file %d)' % b)
        C.check_zero(am[b, K:], what='arg-max, padded atoms')
        C.check_zero(am[b, :, T:], what='arg-max, padded frames')
