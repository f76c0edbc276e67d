"""-m gpu: the time-varying TDOA tracks stage by stage through the C ABI -- track_peaks_kernel, track_carry_kernel
and gcc_steer_kernel<true, false> of csrc/gcc.hip -- at the built inputs of tests/tracks_stage_cases.py, in the conventions of
tests/test_gpu_gcc_stages.py.

The tracks stage is compared EXACTLY, in every frame of every file: the spectrograms are built so that a window sum is exact in float64
in any order (tests/test_tracks_stage_cases_host.py shows it, and that a window off by one frame, the wrong half, the wrong carry or
the wrong tie rule gives other tracks on these very inputs).  The score stage keeps the bounds of tests/gcc_checks.py against float64
and is otherwise compared bit for bit with the fixed-index form, column by column.  No new tolerance anywhere."""
import numpy as np
import pytest

import gcc_checks as C
import tdoa_tracks_restatement as R
import tracks_stage_cases as TC
from gcc_stage_inputs import CELLS, CELL_IDS, cell_seed, geometry, host_file, tuning, upload
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

GARBAGE = 1e30
TRACKS_BIT = 0x100                       # GCCNMF_PEAKS_TRACKS_BIT and GCCNMF_SCORES_TRACKS of include/gccnmf_hip.h
UNWRITTEN = -7


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr()


def round_up(n, m):
    return -(-n // m) * m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the tracks stage -----------------------------------------------------------------------------------------------------------------

def ang_image(spectrograms, D, T, fill):
    """[batch][Dp][Tp] float32 with the files in the corner and ``fill`` in every padded row and frame."""
    img = np.full((len(spectrograms), round_up(D, 64), round_up(T, 64)), fill, np.float32)
    for b, A in enumerate(spectrograms):
        img[b, :D, :T] = A
    return img


def run_tracks(lib, spectrograms, D, T, S, L, fill):
    """One call of the tracks mode on a batch -> (tracks [batch][S][Tp], status [batch][Tp]) as the device left them, -7 where unwritten."""
    B, Tp = len(spectrograms), round_up(T, 64)
    ang = dev(ang_image(spectrograms, D, T, fill))
    tracks = torch.full((B, S, Tp), UNWRITTEN, dtype=torch.int32, device='cuda')
    status = torch.full((B, Tp), UNWRITTEN, dtype=torch.int32, device='cuda')
    word = S | TRACKS_BIT | (L << 9)
    assert 0 < word < 2 ** 31
    assert lib.gccnmf_pick_tdoa_peaks(ptr(ang), D, T, word, B, ptr(tracks), ptr(status), stream()) == 0
    torch.cuda.synchronize()
    return tracks.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('case', range(len(TC.TRACK_CASES)), ids=TC.TRACK_IDS)
def test_tracks_stage_is_the_restatement_exactly(lib, case):
    D, T, S, L, batch, kind = TC.TRACK_CASES[case]
    files = TC.case_files(case)
    spectrograms = [A for _, A, _, _ in files]
    tracks, status = run_tracks(lib, spectrograms, D, T, S, L, float('nan'))
    for b, (pattern, A, want_tracks, want_status) in enumerate(files):
        differ = np.flatnonzero((tracks[b, :, :T] != want_tracks).any(axis=0) | (status[b, :T] != want_status))
        assert len(differ) == 0, ('file %d (%s): %d of %d frames differ, the first at %d: tracks %s status %d, expected %s status %d'
                                  % (b, pattern, len(differ), T, differ[0], tracks[b, :, differ[0]].tolist(), status[b, differ[0]],
                                     want_tracks[:, differ[0]].tolist(), want_status[differ[0]]))
    # frames >= T are not written
    assert (tracks[:, :, T:] == UNWRITTEN).all() and (status[:, T:] == UNWRITTEN).all()
    # nothing outside [0, D) x [0, T) is read into a result: other padding, the same bits
    other = run_tracks(lib, spectrograms, D, T, S, L, GARBAGE)
    assert np.array_equal(other[0], tracks) and np.array_equal(other[1], status), 'the tracks depend on the padding of ang'
    # a file alone gives the bits it gave in the batch
    for b in sorted({0, batch - 1}) if batch > 1 else []:
        alone = run_tracks(lib, [spectrograms[b]], D, T, S, L, float('nan'))
        assert np.array_equal(alone[0][0], tracks[b]) and np.array_equal(alone[1][0], status[b]), 'file %d alone differs' % b
    if not TC.whole_file(T, L):
        return
    # every window is the whole file: constant tracks, those of the whole-file form on the float64 time mean as NumPy computes it
    Dp = round_up(D, 64)
    mean = np.full((batch, Dp), GARBAGE, np.float64)
    for b, A in enumerate(spectrograms):
        mean[b, :D] = np.mean(A.astype(np.float64), axis=1)
    idx = torch.full((batch, S), UNWRITTEN, dtype=torch.int32, device='cuda')
    st = torch.full((batch,), UNWRITTEN, dtype=torch.int32, device='cuda')
    assert lib.gccnmf_pick_tdoa_peaks(ptr(dev(mean)), D, Dp, S, batch, ptr(idx), ptr(st), stream()) == 0
    torch.cuda.synchronize()
    idx, st = idx.cpu().numpy(), st.cpu().numpy()
    normal = 0
    for b in range(batch):
        C.check_peaks(idx[b], st[b], mean[b, :D], S, what='whole-file form, file %d' % b)
        if (status[b, :T] == 0).all():
            normal += 1
            assert st[b] == 0 and np.array_equal(tracks[b, :, :T], np.repeat(idx[b][:, None], T, axis=1)), b
        else:
            assert (status[b, :T] == 3).all() and st[b] == 1, b
    assert normal >= 1


# ---- the score stage with an index per frame --------------------------------------------------------------------------------------------

PAD_INDEXES = np.array([2 ** 31 - 1, -2 ** 31, UNWRITTEN], np.int64)


def tracks_image(tracks, Tp):
    """[batch][S][Tp] int32: the files' (S, T) indexes, the padded frames filled with 2^31 - 1, -2^31 and -7 in turn."""
    B, (S, T) = len(tracks), tracks[0].shape
    img = np.resize(PAD_INDEXES, (B, S, Tp)).astype(np.int32)
    for b, tr in enumerate(tracks):
        img[b, :, :T] = tr
    return img


def run_scores(lib, dv, trig, idx, F, T, K, D, word, B, fill):
    """gccnmf_target_scores_masks over a ``fill``ed workspace and NaN / 0xAB outputs -> host (P, scores, arg-max)."""
    S = word & 0xff
    g = geometry(F, T, K, D)
    nws = lib.gccnmf_scores_workspace_floats(F, T, S, B)
    assert nws == B * g.Fp * S * g.Tp
    ws = torch.full((nws,), fill, dtype=torch.float32, device='cuda')
    scores = torch.full((B, g.Kp, S * g.Tp), float('nan'), dtype=torch.float32, device='cuda')
    am = torch.full((B, g.Kp, g.Tp), 0xAB, dtype=torch.uint8, device='cuda')
    assert lib.gccnmf_target_scores_masks(ptr(dv['CC']), ptr(trig), ptr(idx), ptr(dv['W']), F, T, K, D, word, B, ptr(ws), ptr(scores),
                                          ptr(am), stream()) == 0
    torch.cuda.synchronize()
    return ws.view(B, g.Fp, S, g.Tp).cpu().numpy(), scores.view(B, g.Kp, S, g.Tp).cpu().numpy(), am.cpu().numpy()


def same_bits(a, b, what):
    for name, x, y in zip(('steering product', 'scores', 'arg-max'), a, b):
        assert np.array_equal(x, y, equal_nan=True), '%s: %s differ' % (what, name)


def check_scores_file(P, scores, am, f, tracks, F, T, K, freqs, tdoas, what):
    """One file's (Fp, S, Tp) steering products, (Kp, S, Tp) scores and (Kp, Tp) arg-max against float64 at its per-frame indexes."""
    Cc = f['C'].astype(np.complex128)
    E = R.steering(freqs, tdoas)
    G, Gabs = R.target_scores(f['C'], f['W'], freqs, tdoas, tracks)
    for i in range(tracks.shape[0]):
        e = E[:, tracks[i]]                                                               # (F, T): each frame its own column
        Pabs = np.abs(Cc.real) * np.abs(e.real) + np.abs(Cc.imag) * np.abs(e.imag)
        C.check_gemm_like(P[:F, i, :T], (Cc * e).real, Pabs, 1, what='%s: steering product, target %d' % (what, i))
        C.check_gemm_like(scores[:K, i, :T], G[i], Gabs[i], F, what='%s: scores, target %d' % (what, i))
    C.check_zero(P[F:], what=what + ': steering product, padded bins')
    C.check_zero(P[:, :, T:], what=what + ': steering product, padded frames')
    C.check_zero(scores[:K, :, T:], what=what + ': scores, padded frames')
    C.check_argmax(am[:K, :T], np.transpose(scores[:K, :, :T], (1, 0, 2)), what=what + ': arg-max')
    C.check_zero(am[K:], what=what + ': arg-max, padded atoms')
    C.check_zero(am[:, T:], what=what + ': arg-max, padded frames')


@pytest.mark.parametrize('F,D,S,K,T,batch,key2,key3', list(CELLS), ids=CELL_IDS)
def test_scores_with_an_index_per_frame(lib, F, D, S, K, T, batch, key2, key3):
    from gcc_nmf_amd.engine import steering_tables
    g = geometry(F, T, K, D)
    freqs = O.getFrequenciesInHz(16000, F)
    tdoas = O.getTDOAsInSeconds(1.0, D)
    trig = dev(steering_tables(freqs, tdoas, g.Fp, g.Dp))
    files = [host_file(F, T, K, D, S, cell_seed(F, K, b)) for b in range(batch)]
    drawn = [TC.index_tracks(D, T, S, cell_seed(F, K, b), out_of_range=True) for b in range(batch)]
    own = [TC.index_tracks(D, T, S, cell_seed(F, K, b)) for b in range(batch)]
    tracks, slots, pal = [o[0] for o in own], [o[1] for o in own], own[0][2]
    dv = upload(files, g, S)
    word = S | TRACKS_BIT
    with tuning(lib, key2, key3):
        idx = dev(tracks_image(tracks, g.Tp))
        r = run_scores(lib, dv, trig, idx, F, T, K, D, word, batch, float('nan'))
        again = run_scores(lib, dv, trig, idx, F, T, K, D, word, batch, GARBAGE)
        # the fixed-index form, every target at one slot of its palette: three plain calls
        plain = [run_scores(lib, dv, trig, dev(np.tile(pal[:, j], (batch, 1))), F, T, K, D, S, batch, float('nan')) for j in range(3)]
        alone = {}
        for b in sorted({0, batch - 1}) if batch > 1 else []:
            one = upload([files[b]], g, S)
            alone[b] = run_scores(lib, one, trig, dev(tracks_image([tracks[b]], g.Tp)), F, T, K, D, word, 1, float('nan'))
        # indexes outside [0, D): the bits of the call with the clamped array
        wild = run_scores(lib, dv, trig, dev(tracks_image([d[0] for d in drawn], g.Tp)), F, T, K, D, word, batch, float('nan'))
        clamped = run_scores(lib, dv, trig, dev(tracks_image([d[1] for d in drawn], g.Tp)), F, T, K, D, word, batch, float('nan'))
    same_bits(again, r, 'a workspace of other garbage')
    same_bits(wild, clamped, 'indexes out of range against the clamped ones')
    for b in range(batch):
        what = 'file %d' % b
        check_scores_file(r[0][b], r[1][b], r[2][b], files[b], tracks[b], F, T, K, freqs, tdoas, what)
        check_scores_file(clamped[0][b], clamped[1][b], clamped[2][b], files[b], drawn[b][1], F, T, K, freqs, tdoas, what + ', clamped indexes')
        # column (i, t) carries the bits of the plain call whose slot holds tracks[i, t]
        for j in range(3):
            m = slots[b] == j                                                             # (S, T)
            for name, got, fixed, n in (('steering product', r[0][b], plain[j][0][b], F), ('scores', r[1][b], plain[j][1][b], K)):
                assert np.array_equal(got[:n, :, :T][:, m], fixed[:n, :, :T][:, m]), '%s: %s, columns of slot %d' % (what, name, j)
        assert sum(int((slots[b] == j).sum()) for j in range(3)) == S * T
    # a file's result does not depend on the batch it rides in (same kernels: forced tile policy)
    for b, a in alone.items():
        check_scores_file(a[0][0], a[1][0], a[2][0], files[b], tracks[b], F, T, K, freqs, tdoas, 'file %d alone' % b)
        if key2 != 0:
            same_bits([x[0] for x in a], [x[b] for x in r], 'file %d alone against the batch' % b)


def test_tracks_from_the_device_feed_the_scores_unchanged(lib):
    """The tracks buffer the first stage wrote goes straight into the score call: one stream, no synchronisation and no host round
    trip between the two, the padded frames as the stage left them (-7 here), a status-3 file (tracks -1) in the middle."""
    from gcc_nmf_amd.engine import steering_tables
    F, D, S, K, T, B, L = 129, 33, 2, 96, 65, 3, 5
    g = geometry(F, T, K, D)
    freqs = O.getFrequenciesInHz(16000, F)
    tdoas = O.getTDOAsInSeconds(1.0, D)
    trig = dev(steering_tables(freqs, tdoas, g.Fp, g.Dp))
    built = [TC.build_file(D, T, S, L, kind, pattern, 77 + b) for b, (kind, pattern) in
             enumerate((('grid', 'normal'), ('levels', 'none'), ('levels', 'normal')))]
    files = [host_file(F, T, K, D, S, 4000 + b) for b in range(B)]
    dv = upload(files, g, S)
    ang = dev(ang_image([A for A, _, _ in built], D, T, float('nan')))
    tracks = torch.full((B, S, g.Tp), UNWRITTEN, dtype=torch.int32, device='cuda')
    status = torch.full((B, g.Tp), UNWRITTEN, dtype=torch.int32, device='cuda')
    nws = lib.gccnmf_scores_workspace_floats(F, T, S, B)
    ws = torch.full((nws,), float('nan'), dtype=torch.float32, device='cuda')
    scores = torch.full((B, g.Kp, S * g.Tp), float('nan'), dtype=torch.float32, device='cuda')
    am = torch.full((B, g.Kp, g.Tp), 0xAB, dtype=torch.uint8, device='cuda')
    s = stream()
    assert lib.gccnmf_pick_tdoa_peaks(ptr(ang), D, T, S | TRACKS_BIT | (L << 9), B, ptr(tracks), ptr(status), s) == 0
    assert lib.gccnmf_target_scores_masks(ptr(dv['CC']), ptr(trig), ptr(tracks), ptr(dv['W']), F, T, K, D, S | TRACKS_BIT, B, ptr(ws),
                                          ptr(scores), ptr(am), s) == 0
    torch.cuda.synchronize()
    tracks, status = tracks.cpu().numpy(), status.cpu().numpy()
    r = (ws.view(B, g.Fp, S, g.Tp).cpu().numpy(), scores.view(B, g.Kp, S, g.Tp).cpu().numpy(), am.cpu().numpy())
    for b, (A, want_tracks, want_status) in enumerate(built):
        assert np.array_equal(tracks[b, :, :T], want_tracks) and np.array_equal(status[b, :T], want_status), b
    assert (tracks[:, :, T:] == UNWRITTEN).all() and (status[1, :T] == 3).all() and (tracks[1, :, :T] == -1).all()
    assert all((status[b, :T] == 0).any() and (status[b, :T] == 1).any() for b in (0, 2))
    # the normal files at their tracks; the status-3 file as index 0, the header's clamping rule
    scored_at = [built[0][1], np.zeros((S, T), np.int32), built[2][1]]
    for b in range(B):
        check_scores_file(r[0][b], r[1][b], r[2][b], files[b], scored_at[b], F, T, K, freqs, tdoas, 'file %d' % b)
    # and bit for bit what the same indexes give when a host uploads them, -1 written as 0
    uploaded = run_scores(lib, dv, trig, dev(tracks_image(scored_at, g.Tp)), F, T, K, D, S | TRACKS_BIT, B, float('nan'))
    same_bits(r, uploaded, 'device-written tracks against uploaded ones')
    zero = run_scores(lib, dv, trig, dev(np.zeros((B, S), np.int32)), F, T, K, D, S, B, float('nan'))
    same_bits([x[1] for x in r], [x[1] for x in zero], 'the status-3 file against the plain form at index 0')
