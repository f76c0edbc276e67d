"""Scoring on the device against the float64 restatement (tests/bss_eval_restatement.py): the two kernels of
libgccnmf_eval.so element by element within their derived bars, bit for bit the same for a file alone and inside a batch, the four
criteria and the permutation of gcc_nmf_amd.evaluation.bss_eval_images, GCCNMFEngine.score, and a silent true source.

Shapes (J, C, n, L), R.SHAPES: the five of the issue, n = the correlation kernel's block length + 1, n below L, and three that cross the
edges of the kernels' own tiles -- (2,2,1500,70): taps beyond 64, so every operand slot of the 16 x 8 register tile carries data, on four
reference signals; (1,2,4200,130): more than 4096 output samples (a second output block of the projection kernel) and five correlation
blocks; (1,1,1300,520): more than 512 taps (a second staging pass of the projection kernel) and more than 1024 lags (a second lag chunk of
the correlation kernel, and in the symmetric call a skipped one).  Together they cover odd L, L across a 16-lag tile edge (33), ragged last
blocks, a single source and a single channel.  Every shape is three files (seeds 0, 1, 2; the third with its estimates in reverse
order): batches of 1 and 3.  A batch cut into three chunks of files (odd n: chunks that start off a 16-byte boundary) has its own test."""
import warnings

import numpy as np
import pytest

import bss_eval_restatement as R

pytestmark = pytest.mark.gpu

SHAPES = R.SHAPES
IDS = ['J%d-C%d-n%d-L%d' % s for s in SHAPES]
_cache = {}
_tables = {}


def restatement_tables(shape, f):
    """The restatement's four (J_est, J_true) tables and cond(G) of file f of a shape, computed once."""
    if (shape, f) not in _tables:
        s, e = R.case_files(shape)[f]
        _tables[shape, f] = R.all_pairs(s, e, shape[3])
    return _tables[shape, f]


def device_case(shape):
    """Everything the tests of one shape share, computed once: the three files, and from the device, for the batch of 3 and for file 2
    alone, both lag correlations, the projection filters (the device's own) and the projections."""
    if shape in _cache:
        return _cache[shape]
    import torch
    from gcc_nmf_amd import _eval, evaluation
    J, C, n, L = shape
    assert _eval.GCCNMF_EVAL_BLOCK == 1024
    files = R.case_files(shape)
    pairs = [(j, i) for j in range(J) for i in range(J)]
    out = dict(files=files, pairs=pairs)
    with torch.cuda.device(0):
        dev = torch.device('cuda:0')
        ranges = evaluation.projection_ranges(J, C, pairs, dev)
        out['ranges'] = ranges.cpu().numpy()
        for name, pick in (('batch', [0, 1, 2]), ('alone', [1])):
            A = torch.from_numpy(np.stack([files[k][0] for k in pick]).reshape(len(pick), J * C, n)).to(dev)
            Et = torch.from_numpy(np.stack([files[k][1] for k in pick]).reshape(len(pick), J * C, n)).to(dev)
            Rss, Rse = _eval.lag_correlations(A, A, L), _eval.lag_correlations(A, Et, L)
            if name == 'batch':
                coef, failed = evaluation.projection_coefficients(A, Et, J, L, pairs)
                assert not bool(failed.any())
                out['coef'] = coef.cpu().numpy()
                P = _eval.project(A, coef, ranges)
            else:
                P = _eval.project(A, coef[1:2].clone(), ranges)
            torch.cuda.synchronize()
            out[name] = dict(Rss=Rss.cpu().numpy(), Rse=Rse.cpu().numpy(), P=P.cpu().numpy())
    _cache[shape] = out
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_lag_correlations_within_the_bar(shape):
    """|R_dev - R_exact| <= m 2^-53 sum |a_n b_{n+l}| for every element, the mirrored half of the symmetric call included; the symmetric
    call's R is symmetric to the bit."""
    J, C, n, L = shape
    case = device_case(shape)
    for f, (s, e) in enumerate(case['files']):
        A, B = s.reshape(J * C, n), e.reshape(J * C, n)
        for name, other in (('Rss', A), ('Rse', B)):
            exact, bar = R.lag_correlations_exact(A, other, L)
            err = np.abs(case['batch'][name][f] - exact)
            assert (err <= bar).all(), (name, f, float((err / np.maximum(bar, 1e-300)).max()))
        Rss = case['batch']['Rss'][f]
        assert np.array_equal(Rss, Rss.transpose(1, 0, 2)[:, :, ::-1])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_projections_within_the_bar(shape):
    """|P_dev - P_ref| <= (t + 2) 2^-53 sum |coef| |s| for every element, against the restatement fed the device's own coefficients."""
    J, C, n, L = shape
    case = device_case(shape)
    for f, (s, _) in enumerate(case['files']):
        ref, bar = R.projections_reference(s.reshape(J * C, n), case['coef'][f], case['ranges'])
        err = np.abs((case['batch']['P'][f].astype(np.longdouble) - ref).astype(np.float64))
        assert (err <= bar).all(), (f, float((err / np.maximum(bar, 1e-300)).max()))
        assert np.abs(case['batch']['P'][f]).max() > 0


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_a_file_alone_and_as_file_2_of_3_agree_bit_for_bit(shape):
    case = device_case(shape)
    for name in ('Rss', 'Rse', 'P'):
        assert np.array_equal(case['alone'][name][0], case['batch'][name][1]), name


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_criteria_and_permutation_against_the_restatement(shape, batch):
    """SDR, ISR, SIR, SAR within R.DB_TOLERANCE of the restatement (cond(G) < 1e3 asserted first), +inf where it has +inf, perm equal; the
    all-pairs tables and the fixed assignment likewise."""
    from gcc_nmf_amd.evaluation import bss_eval_images
    J, C, n, L = shape
    files = R.case_files(shape)[:batch]
    s, e = np.stack([f[0] for f in files]), np.stack([f[1] for f in files])
    if batch == 1:
        s, e = s[0], e[0]
    got = bss_eval_images(s, e, L)
    tables = bss_eval_images(s, e, L, allPairs=True)
    fixed = bss_eval_images(s, e, L, computePermutation=False)
    assert got[0].shape == ((J,) if batch == 1 else (batch, J)) and tables[0].shape == ((J, J) if batch == 1 else (batch, J, J))
    assert len(got) == 5 and len(tables) == 4 and len(fixed) == 5

    def close(x, y):
        inf = np.isposinf(y)
        assert np.array_equal(np.isposinf(x), inf) and np.isfinite(y[~inf]).all(), (x, y)
        worst = float(np.abs(x[~inf] - y[~inf]).max(initial=0.0))
        print('%s batch %d: largest difference %.3e dB' % (shape, batch, worst))
        assert worst <= R.DB_TOLERANCE, worst

    for f, (sf, ef) in enumerate(files):
        want_tables = restatement_tables(shape, f)
        assert want_tables[4] < 1e3
        want_perm, true = R.best_permutation(want_tables[2]), np.arange(J)
        want = tuple(t[want_perm, true] for t in want_tables[:4]) + (want_perm,)
        want_fixed = tuple(t[true, true] for t in want_tables[:4])
        at = (lambda v: v) if batch == 1 else (lambda v: v[f])
        for k in range(4):
            close(at(got[k]), want[k])
            close(at(tables[k]), want_tables[k])
            close(at(fixed[k]), want_fixed[k])
        assert at(got[4]).tolist() == want[4].tolist() and at(fixed[4]).tolist() == list(range(J))
        if f == 2:
            assert want[4].tolist() == list(range(J))[::-1]
    if J == 1:
        assert np.isposinf(got[2]).all()


def test_a_batch_cut_into_three_chunks_of_files_gives_the_one_chunk_figures():
    """7 files of (3, 1, 1001) under a cap of 3 files per chunk: chunks of 3, 3 and 1 files that start 36036 and 72072 bytes into the
    batch, neither a multiple of 16 (the kernels take 16-byte aligned pointers: such a chunk is copied).  The criteria agree with the
    run in one chunk within R.DB_TOLERANCE (the kernels' parts are the same bits; the batched solve may round differently), and with
    the restatement for a file of each chunk."""
    import torch
    from gcc_nmf_amd import evaluation
    J, C, n, L, B = R.CHUNKED
    assert (J, C, n, L, B) == (3, 1, 1001, 16, 7)
    files =[R.make_case(J, C, n, L, seed=k) for k in range(B)]
    cap = 3 * evaluation.GRAM_COPIES * 8 * (J * C * L) ** 2
    assert evaluation.files_per_chunk(J, C, L, cap) == 3 and evaluation.files_per_chunk(J, C, L) >= B
    assert (3 * J * C * n * 4) % 16 and (6 * J * C * n * 4) % 16
    pairs = [(j, i) for j in range(J) for i in range(J)]
    with torch.cuda.device(0):
        S = torch.from_numpy(np.stack([f[0] for f in files])).to('cuda:0')
        E = torch.from_numpy(np.stack([f[1] for f in files])).to('cuda:0')
        assert evaluation._aligned_chunk(S, 3, 3).data_ptr() % 16 == 0 and S[3:6].data_ptr() % 16
        whole, status_whole = evaluation.pair_energies(S, E, L, pairs)
        cut, status_cut = evaluation.pair_energies(S, E, L, pairs, gram_cap_bytes=cap)
    assert not status_whole.any() and not status_cut.any()
    one = evaluation.criteria_from_energies(whole.reshape(B, J, J, 7))
    three = evaluation.criteria_from_energies(cut.reshape(B, J, J, 7))
    for k in range(4):
        worst = float(np.abs(one[k] - three[k]).max())
        print('criterion %d: three chunks against one, largest difference %.3e dB' % (k, worst))
        assert np.isfinite(one[k]).all() and worst <= R.DB_TOLERANCE
    for f in (1, 4, 6):
        want = R.all_pairs(files[f][0], files[f][1], L)
        assert want[4] < 1e3
        for k in range(4):
            assert np.abs(three[k][f] - want[k]).max() <= R.DB_TOLERANCE


def test_a_silent_true_source_gives_status_1():
    """Status 1, NaN for ISR, SIR and SAR, one warning; SDR is still the plain energy ratio: finite for the sources that sound, and
    10 log10(0 / |e|^2) = -inf for the silent one itself."""
    from gcc_nmf_amd.evaluation import bss_eval_images
    s, e = R.make_case(3, 2, 1000, 16)
    good = R.make_case(3, 2, 1000, 16, seed=1)
    s[1] = 0
    S, E = np.stack([s, good[0]]), np.stack([e, good[1]])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        sdr, isr, sir, sar, perm, status = bss_eval_images(S, E, 16, returnStatus=True)
    assert len([w for w in caught if 'could not be solved' in str(w.message)]) == 1
    assert status.tolist() == [1, 0] and perm[0].tolist() == [0, 1, 2]
    assert np.isnan(isr[0]).all() and np.isnan(sir[0]).all() and np.isnan(sar[0]).all()
    assert np.isfinite(sdr[0][[0, 2]]).all() and np.isneginf(sdr[0][1])
    s64, e64 = s.astype(np.float64), e.astype(np.float64)
    for i in (0, 2):
        assert abs(sdr[0][i] - 10 * np.log10(np.sum(s64[i] ** 2) / np.sum((e64[i] - s64[i]) ** 2))) < 1e-9
    want = R.bss_eval_images(good[0], good[1], 16)
    for k in range(4):
        assert np.abs(np.stack([sdr, isr, sir, sar])[k][1] - want[k]).max() <= R.DB_TOLERANCE


def test_engine_score_against_bss_eval_images_on_the_downloaded_waveforms():
    """GCCNMFEngine.score scores the waveforms where they lie: the same figures as bss_eval_images on the downloaded waveforms and the
    images cut to them (y[n] belongs to images[..., n + windowSize // 2]; guardSamples cut at both ends).  Also the enhancement engine
    (S = 2), and the ValueErrors."""
    import torch
    from gcc_nmf_amd.engine import GCCNMFEngine, GCCNMFEnhancementEngine
    from gcc_nmf_amd.evaluation import bss_eval_images
    from gcc_nmf_amd.synthetic import reverberant_mixture
    n, L, guard = 16000, 24, 300
    made = [reverberant_mixture(50 + b, numSamples=n, returnSources=True) for b in range(2)]
    xs = np.stack([m[0] for m in made])
    rng = np.random.default_rng(11)
    # the images are low-passed: an independent white component keeps their Gram matrix well conditioned
    images = np.stack([m[1] + 0.3 * m[1].std() * rng.standard_normal(m[1].shape) for m in made]).astype(np.float32)
    with torch.cuda.device(0):
        eng = GCCNMFEngine(n, dictionarySize=32, numIterations=10, batch=2, device='cuda:0')
        with pytest.raises(ValueError, match='separation first'):
            eng.score(images, filterLength=L)
        y = eng.separate(xs)
        got = eng.score(images, filterLength=L, guardSamples=guard)
        again = eng.score(torch.from_numpy(images), filterLength=L, guardSamples=guard)
        off, Ly = eng.n_fft // 2, y.shape[-1]
        want = bss_eval_images(images[..., off + guard:off + Ly - guard], y[..., guard:Ly - guard], L)
        assert np.isfinite(np.stack(got[:4])).all() and np.array_equal(got[4], want[4]) and np.array_equal(again[4], want[4])
        for k in range(4):                   # the same arithmetic on the same samples: R.DB_TOLERANCE is generous
            assert got[k].shape == (2, 3) and np.abs(got[k] - want[k]).max() <= R.DB_TOLERANCE and np.abs(again[k] - want[k]).max() <= R.DB_TOLERANCE
        whole = eng.score(images, filterLength=L)
        assert np.abs(whole[0] - bss_eval_images(images[..., off:off + Ly], y, L)[0]).max() <= R.DB_TOLERANCE
        for bad in (dict(guardSamples=-1), dict(guardSamples=Ly), dict(guardSamples=1.5), dict(filterLength=0), dict(filterLength=4097)):
            with pytest.raises(ValueError):
                eng.score(images, **bad)
        with pytest.raises(ValueError):
            eng.score(images[:, :2])
        nan = images.copy()
        nan[1, 0, 0, 5000] = np.nan
        with pytest.raises(ValueError):
            eng.score(nan)
        auto = GCCNMFEngine(n, dictionarySize=32, numIterations=10, batch=2, numTargets='auto', device='cuda:0')
        with pytest.raises(ValueError):
            auto.score(np.zeros((2, 4, 2, n), np.float32))
        enh = GCCNMFEnhancementEngine(n, dictionarySize=32, numIterations=10, batch=2, device='cuda:0')
        y2 = enh.separate(xs)
        two = np.stack([images[:, 0], images[:, 1] + images[:, 2]], axis=1)
        got2 = enh.score(two, filterLength=L, guardSamples=guard)
        want2 = bss_eval_images(two[..., off + guard:off + Ly - guard], y2[..., guard:Ly - guard], L)
        assert np.array_equal(got2[4], want2[4])
        for k in range(4):
            assert got2[k].shape == (2, 2) and np.isfinite(got2[k]).all() and np.abs(got2[k] - want2[k]).max() <= R.DB_TOLERANCE
