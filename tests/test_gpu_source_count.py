"""-m gpu: numSources='auto'  -- the count mode of gccnmf_pick_tdoa_peaks (csrc/source_count.hip) against the NumPy
restatement in tests/source_count_restatement.py, exactly; the counted mode of gccnmf_target_scores_masks (absent targets: NaN scores,
never the arg-max); absent targets through the three reconstructions and the inverse STFT (exactly zero); the engines and the named
functions end to end on mixtures of one to five talkers."""
import numpy as np
import pytest

import gcc_checks as C
import source_count_restatement as SC
from conftest import golden
from oracle import gccnmf_oracle as O
from test_gpu_gcc_stages import GARBAGE, geometry, host_file, nan_like, ptr, stream, tuning, upload
from test_source_count_host import MIXTURES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ERR_ARG = 1
COUNT_BIT = 1 << 30
COUNTED = 0x800
U = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


# ---- the count mode ---------------------------------------------------------------------------------------------------------------
def embed(heights, D, gap=0.0):
    """Peaks of the given heights at 1, 3, 5, ... of a D-point spectrum, ``gap`` everywhere else."""
    v = np.full(D, gap, np.float64)
    v[1:2 * len(heights):2] = heights
    return v


def built_spectra(D, rng, files=70):
    """Spectra as tests/test_gpu_gcc_stages.py builds them for the fixed count, and the count's own edge cases; ``files`` in all."""
    out = [np.arange(D, dtype=np.float64), -np.arange(D, dtype=np.float64), np.zeros(D)]             # monotone / flat: no peak
    out += [embed([1.0], D), embed([np.inf], D)]                                                          # one peak, whatever its height
    three = rng.randint(0, 3, (6, D)).astype(np.float64)                                                  # three levels: ties everywhere
    out += list(three)
    if D >= 5:
        out += [embed([1.0, 1.0], D), embed([2.0, 1.0], D), embed([np.inf, 1.0], D), embed([1e308, 1e308], D)]
        alt = np.zeros(D)
        alt[1::2] = 1.0                                                                                   # all peaks equal, as many as fit
        alt[D - 1] = 0.0
        out += [alt, 7.0 * alt, alt * 1e-300]
    if D >= 9:
        out += [embed([3.0, 2.0, 1.0], D), embed([1.0, 3.0, 2.0], D), embed([2.0, 2.0, 0.0, 2.0], D, gap=-1.0)]      # the worked examples
        p = rng.standard_normal(D)
        p[3] = p[4] = 9.0                                                                                 # plateau: not a strict maximum
        out.append(p)
    if D >= 64:
        for run in (1, 5, 17):                                                                            # NaN runs
            v = rng.standard_normal(D)
            at = rng.randint(1, D - run)
            v[at:at + run] = np.nan
            out.append(v)
        v = rng.standard_normal(D)
        v[0] = v[D - 1] = np.nan
        out.append(v)
        t = np.zeros(D)
        t[[3, 9, 20, 33, 50, 61]] = 5.0                                                                   # six equal peaks over a floor ...
        t[[12, 40]] = 1.0                                                                                 # ... and two low ones: count 6
        out.append(t)
        lv = rng.standard_normal(D) * 1e-3
        lv[rng.choice(np.arange(1, D - 1, 2), min(12, D // 4), replace=False)] += 1.0                     # up to 12 talkers: the cap
        out.append(lv)
    while len(out) < files:
        scale = (1.0, 1e150, 1e-200)[len(out) % 3]
        out.append(rng.standard_normal(D) * scale + (len(out) % 2))
    return out[:files]


def device_count(mean, D, Dp, Smax, batch):
    from gcc_nmf_amd import _hip
    idx = torch.full((batch, Smax), -7, dtype=torch.int32, device='cuda')
    st = torch.full((batch,), -7, dtype=torch.int32, device='cuda')
    _hip.count_tdoa_peaks(mean, D, Dp, Smax, batch, idx, st)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize('D', [3, 5, 64, 65, 128, 1000, 4096])
def test_count_mode_is_the_restatement_exactly(lib, D):
    rng = np.random.RandomState(100 + D)
    spectra = built_spectra(D, rng)
    B, Dp = len(spectra), -(-D // 64) * 64
    assert B == 70
    m = np.full((B, Dp), GARBAGE)                                      # padding beyond D must not be read
    for b, v in enumerate(spectra):
        m[b, :D] = v
    dm = torch.from_numpy(m).cuda()
    host = dm.cpu().numpy()                                            # the device's own float64 input
    seen = set()
    for Smax in (1, 4, 8, 255):
        idx, st = device_count(dm, D, Dp, Smax, B)
        for b in range(B):
            want, status = SC.count_sources(host[b, :D], Smax)
            assert (idx[b].tolist(), int(st[b])) == (want, status), (D, Smax, b, idx[b][:12].tolist(), int(st[b]), want[:12], status)
            seen.add(status)
        # a file alone gives the words it gives inside the batch (its own row only)
        for b in (0, 7, B - 1):
            alone_idx, alone_st = device_count(dm[b], D, Dp, Smax, 1)
            assert np.array_equal(alone_idx[0], idx[b]) and alone_st[0] == st[b], (D, Smax, b)
    assert seen == ({0, 1} if D < 64 else {0, 1, 2})                   # every status was reached


def test_mode_word_hygiene(lib):
    D, Dp, B, S = 128, 128, 2, 4
    rng = np.random.RandomState(3)
    dm = torch.from_numpy(rng.standard_normal((B, Dp))).cuda()
    idx = torch.full((B, S), -7, dtype=torch.int32, device='cuda')
    st = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    call = lambda word, Dn=D, Dpn=Dp, Bn=B, m=dm: lib.gccnmf_pick_tdoa_peaks(ptr(m) if m is not None else 0, Dn, Dpn, word, Bn, ptr(idx), ptr(st), stream())
    for word in (COUNT_BIT, S | COUNT_BIT | 0x200, S | COUNT_BIT | (1 << 29), S | COUNT_BIT | (1 << 9), -(S | COUNT_BIT), S | (1 << 31) - (1 << 32) | COUNT_BIT):
        assert call(word) == ERR_ARG, hex(word)
    # the count bit together with bit 8 is a tracks word (bit 30 is bit 21 of its window length) whose Dp slot carries T: called with
    # Dp = 2^21, which the count mode would take and the tracks mode rejects, so that neither kernel can run over these buffers
    assert call(S | COUNT_BIT | 0x100, Dpn=1 << 21, Bn=1) == ERR_ARG
    for Dn, Dpn, Bn, m in ((2, 64, B, dm), (4097, 4160, B, dm), (128, 64, B, dm), (D, Dp, 0, dm), (D, Dp, B, None)):      # what the plain form rejects
        assert call(S | COUNT_BIT, Dn, Dpn, Bn, m) == ERR_ARG, (Dn, Dpn, Bn)
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all() and (st.cpu().numpy() == -7).all()     # a rejected call writes nothing
    # the plain form on the same buffers: today's results
    assert call(S) == 0
    torch.cuda.synchronize()
    for b in range(B):
        C.check_peaks(idx.cpu().numpy()[b], st.cpu().numpy()[b], dm.cpu().numpy()[b, :D], S)
    assert call(S | COUNT_BIT) == 0
    torch.cuda.synchronize()
    for b in range(B):
        assert (idx.cpu().numpy()[b].tolist(), int(st.cpu().numpy()[b])) == SC.count_sources(dm.cpu().numpy()[b, :D], S)

    # the scores call: the counted bit with any other mode is rejected before anything is written
    F, T, K, Ds = 33, 5, 5, 64
    g = geometry(F, T, K, Ds)
    dv = upload([host_file(F, T, K, Ds, S, 1)], g, S)
    trig = steering(F, Ds, g)
    ws = torch.full((lib.gccnmf_scores_workspace_floats(F, T, S, 1),), GARBAGE, dtype=torch.float32, device='cuda')
    scores = torch.full((1, g.Kp, S * g.Tp), GARBAGE, dtype=torch.float32, device='cuda')
    am = torch.full((1, g.Kp, g.Tp), 0xAB, dtype=torch.uint8, device='cuda')
    sc = lambda word: lib.gccnmf_target_scores_masks(ptr(dv['CC']), ptr(trig), ptr(dv['tdoa']), ptr(dv['W']), F, T, K, Ds, word, 1, ptr(ws),
                                                     ptr(scores), ptr(am), stream())
    for word in (COUNTED | 0x100 | S, COUNTED | 0x200 | S, COUNTED | 0x400 | S, COUNTED | 0x200, COUNTED, COUNTED | (1 << 16) | S, -(COUNTED | S)):
        assert sc(word) == ERR_ARG, hex(word)
    torch.cuda.synchronize()
    assert (scores.cpu().numpy() == np.float32(GARBAGE)).all() and (am.cpu().numpy() == 0xAB).all() and (ws.cpu().numpy() == np.float32(GARBAGE)).all()
    assert sc(S) == 0 and sc(S | COUNTED) == 0
    torch.cuda.synchronize()


# ---- the counted scores -----------------------------------------------------------------------------------------------------------
def steering(F, D, g):
    from gcc_nmf_amd.engine import steering_tables
    return torch.from_numpy(steering_tables(O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D), g.Fp, g.Dp)).cuda()


ROWS = np.array([[9, 20, 40, 55], [9, -1, -1, -1], [-1, 30, -1, 50]], np.int32)


def run_scores(lib, dv, trig, g, D, S, B, word):
    ws = torch.full((lib.gccnmf_scores_workspace_floats(g.F, g.T, S, B),), GARBAGE, dtype=torch.float32, device='cuda')
    scores = nan_like((B, g.Kp, S * g.Tp))
    am = torch.full((B, g.Kp, g.Tp), 0xAB, dtype=torch.uint8, device='cuda')
    assert lib.gccnmf_target_scores_masks(ptr(dv['CC']), ptr(trig), ptr(dv['tdoa']), ptr(dv['W']), g.F, g.T, g.K, D, word, B, ptr(ws), ptr(scores),
                                          ptr(am), stream()) == 0
    torch.cuda.synchronize()
    return scores.view(B, g.Kp, S, g.Tp).cpu().numpy(), am.cpu().numpy()


@pytest.mark.parametrize('K', [5, 70, 130])
@pytest.mark.parametrize('T', [1, 5, 63, 65, 130])
def test_counted_scores(lib, T, K):
    F, D, S, B = 33, 64, 4, 3
    g = geometry(F, T, K, D)
    freqs, tdoas = O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D)
    E = np.exp(np.outer(freqs, -(2j * np.pi) * tdoas))
    files = [host_file(F, T, K, D, S, 7000 + 100 * T + K + b) for b in range(B)]
    for b, f in enumerate(files):
        f['tdoa'] = ROWS[b]
    dv = upload(files, g, S)
    trig = steering(F, D, g)
    for policy in (0, 1):                  # by size (one small launch: the ring tile) and the throughput tiles (K > 128 picks the other one)
        with tuning(lib, policy, 1):
            scores, am = run_scores(lib, dv, trig, g, D, S, B, S | COUNTED)
            plain, plain_am = run_scores(lib, dv, trig, g, D, S, B, S)
        for b, f in enumerate(files):
            Cc, W64 = f['C'].astype(np.complex128), f['W'].astype(np.float64)
            for i, tau in enumerate(ROWS[b]):
                got = scores[b, :K, i, :T]
                if tau < 0:
                    assert np.isnan(got).all(), ('absent target %d of file %d has numbers' % (i, b), policy)
                    continue
                e = E[:, tau][:, None]
                Pabs = np.abs(Cc.real) * np.abs(e.real) + np.abs(Cc.imag) * np.abs(e.imag)
                C.check_gemm_like(got, np.dot(W64.T, (Cc * e).real), np.dot(np.abs(W64).T, Pabs), F, what='scores, file %d target %d' % (b, i))
            C.check_zero(scores[b, :K, :, T:], what='scores, padded frames (file %d)' % b)       # of absent targets too
            C.check_argmax(am[b, :K, :T], np.transpose(scores[b, :K, :, :T], (1, 0, 2)), what='arg-max (file %d)' % b)
            assert np.isin(am[b, :K, :T], np.nonzero(ROWS[b] >= 0)[0]).all()                    # an absent target owns no atom
            C.check_zero(am[b, K:], what='arg-max, padded atoms')
            C.check_zero(am[b, :, T:], what='arg-max, padded frames')
        # a row of non-negative indexes: the plain mode's bits
        assert np.array_equal(scores[0], plain[0], equal_nan=True) and np.array_equal(am[0], plain_am[0]), policy


# ---- absent targets through the reconstruction and the inverse STFT ---------------------------------------------------------------
@pytest.mark.parametrize('reconstruction', ['direct', 'ratio', 'spatial'])
def test_absent_slots_are_exactly_zero(lib, reconstruction):
    from gcc_nmf_amd.engine import GCCNMFEngine
    n_fft, hop, T, K, S, B = 64, 16, 65, 70, 4, 3
    n = n_fft + hop * (T - 1)
    x = (0.1 * np.random.RandomState(11).standard_normal((B, 2, n))).astype(np.float32)
    e = GCCNMFEngine(n, windowSize=n_fft, hopSize=hop, numTDOAs=64, numTargets='auto', maxTargets=S, dictionarySize=K, numIterations=5,
                     batch=B, reconstruction=reconstruction)
    assert (e.g.F, e.g.T, e.g.S) == (33, T, S)
    e.upload(x)
    e.stft()
    e.klnmf()
    e.localize()
    e.tdoa_idx.copy_(torch.from_numpy(ROWS))                           # the files' targets, given: present and absent slots
    e.masks()
    e.spec.fill_(float('nan'))
    e.y.fill_(float('nan'))
    e.reconstruct()
    e.istft()
    torch.cuda.synchronize()
    assert e.get_num_sources().tolist() == [4, 1, 2]
    spec, y, X = e.get_spec(), e.y.cpu().numpy(), e.get_X()
    present = ROWS >= 0
    for b in range(B):
        for i in range(S):
            if present[b, i]:
                assert np.isfinite(spec[b, i]).all() and np.abs(spec[b, i]).max() > 0 and np.isfinite(y[b, i]).all() and np.abs(y[b, i]).max() > 0
            else:
                assert np.isfinite(spec[b, i]).all() and (np.abs(spec[b, i]) == 0).all(), (reconstruction, b, i)
                assert (y[b, i] == 0).all(), (reconstruction, b, i)
    if reconstruction == 'ratio':
        # the present targets still add up to the mixture: the partition bound of tests/test_gpu_ratio_reconstruction.py, S slots
        err = spec.astype(np.complex128).sum(axis=1) - X
        worst = float((np.abs(err) / ((3 * S + 2) * U * np.abs(X))).max())
        print('ratio mode with absent targets: partition %.3g of the (3S+2)u|X| bound' % worst)
        assert worst <= 1


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def mixtures():
    from gcc_nmf_amd.synthetic import synthetic_mixture
    cases = [(0, d) for d, _ in MIXTURES] + [(1, d) for d, _ in MIXTURES[:3]]
    return np.stack([synthetic_mixture(i, 32000, 16000, delays=d) for i, d in cases])


def check_slots(y, counts, what):
    assert np.isfinite(y).all(), what
    for b, n in enumerate(counts):
        assert (y[b, n:] == 0).all(), (what, b)
        for i in range(n):
            assert np.abs(y[b, i]).max() > 0, (what, b, i)


def test_engine_separates_files_of_different_counts():
    from gcc_nmf_amd.engine import GCCNMFEngine
    xs = mixtures()
    e = GCCNMFEngine(32000, numTargets='auto', maxTargets=4, dictionarySize=32, numIterations=20, batch=8)
    y = e.separate(xs)                                                 # check_status() inside: the capped file does not raise
    assert y.shape == (8, 4, 2, e.L)
    counts, idx, status = e.get_num_sources(), e.get_tdoa_indexes(), e.get_count_status()
    mean = e.get_angular()[1]
    for b in range(8):
        assert (idx[b].tolist(), int(status[b])) == SC.count_sources(mean[b], 4), b
    assert counts.tolist() == [1, 2, 3, 4, 4, 1, 2, 3] and counts.dtype == np.int64
    assert status.tolist() == [0, 0, 0, 0, 2, 0, 0, 0]
    assert idx.shape == (8, 4) and [idx[b, :n].tolist() for b, n in enumerate(counts[:4])] == [p for _, p in MIXTURES[:4]]
    e.check_status()
    check_slots(y, counts, 'separate')
    # the other two outputs
    yb = next(e.separate_batches([xs]))
    assert yb.shape == y.shape
    check_slots(yb, counts, 'separate_batches')
    pcm = e.separate_pcm16(np.ascontiguousarray((xs * 32768).astype(np.int16).transpose(0, 2, 1)))
    assert pcm.shape == (8, 4, e.L, 2)
    check_slots(pcm.astype(np.float32), counts, 'separate_pcm16')
    # the three-talker file: the peaks a numTargets=3 engine picks on it
    e3 = GCCNMFEngine(32000, numTargets=3, dictionarySize=32, numIterations=20, batch=1)
    e3.separate(xs[2:3])
    assert e3.get_tdoa_indexes()[0].tolist() == idx[2, :3].tolist() == [27, 59, 91]
    assert e3.get_num_sources().tolist() == [3]
    with pytest.raises(ValueError):
        e3.get_count_status()
    # a file without any peak is the one failure: file_status() / check_status() report it, a capped count they do not
    e.status.copy_(torch.tensor([0, 2, 1, 0, 2, 0, 0, 1], dtype=torch.int32))
    assert e.file_status().cpu().numpy().tolist() == [0, 0, 1, 0, 0, 0, 0, 1]
    with pytest.raises(ValueError, match=r'file\(s\) \[2, 7\]'):
        e.check_status()


def test_ragged_engine_counts_per_file():
    from gcc_nmf_amd.engine import GCCNMFEngine, RaggedGCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_mixture
    lengths = [32000, 48000]
    xs = [synthetic_mixture(0, 32000, 16000, delays=(-20, 27)), synthetic_mixture(0, 48000, 16000, delays=(-20, 3, 27))]
    e = GCCNMFEngine(lengths=lengths, numTargets='auto', maxTargets=4, dictionarySize=32, numIterations=20)
    assert isinstance(e, RaggedGCCNMFEngine)
    ys = e.separate(xs)
    assert e.get_num_sources().tolist() == [2, 3]
    for y, n, L in zip(ys, (2, 3), lengths):
        assert y.shape == (4, 2, 256 * (1 + (L - 1024) // 256 - 1))
        check_slots(y[None], [n], 'ragged')


def test_named_functions():
    from gcc_nmf_amd import gccNMFFunctions as G
    dev1 = golden('dev1_hop256_K128')
    got = G.estimateTargetTDOAIndexesFromAngularSpectrum(dev1['meanA'], 1.0, 128, 'auto')
    assert got == dev1['idx'].tolist() and len(got) == 3 and all(isinstance(i, np.int64) for i in got)
    assert G.estimateNumSourcesFromAngularSpectrum(dev1['meanA']) == (3, got, 0)
    count, kept, status = G.estimateNumSourcesFromAngularSpectrum(dev1['meanA'], maxSources=2)
    assert (count, status) == (2, 2) and kept == SC.count_sources(dev1['meanA'], 2)[0]
    assert G.estimateNumSourcesFromAngularSpectrum(np.arange(128.0)) == (0, [], 1)
    with pytest.raises(ValueError, match="didn't find enough peaks"):
        G.estimateTargetTDOAIndexesFromAngularSpectrum(np.arange(128.0), 1.0, 128, 'auto')
    with pytest.raises(ValueError):
        G.estimateTargetTDOAIndexesFromAngularSpectrum(dev1['meanA'], 1.0, 128, None)
    # the three-step wrapper, and what the count feeds
    from gcc_nmf_amd.synthetic import synthetic_mixture
    X = O.computeComplexMixtureSpectrogram(synthetic_mixture(0, 32000, 16000, delays=(-20, 27)), 1024, 256, np.hanning)
    found, meanA = G.getTargetTDOAEstimates(X, 16000, 1.0, 128, numSources='auto')
    assert found == [27, 91] and found == SC.count_sources(meanA, G.MAX_AUTO_SOURCES)[0][:2]
