"""The stage layer of gcc_nmf_amd._hip: the exact integers that reach the C ABI for every mode keyword.  No device, no library: a
recording stub stands in for the loaded shared object."""
import ctypes

import pytest
import torch

from gcc_nmf_amd import _hip

STREAM = 0x5eed


class StubLibrary(object):
    """Every attribute is an entry point that records (name, args) and returns ``status``."""

    def __init__(self, status=0, chain_word=0):
        self.calls, self.status, self.chain_word = [], status, chain_word

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if name == 'gccnmf_klnmf_chain_status':
                args[-1]._obj.value = self.chain_word
            return 4321 if name.endswith('_workspace_floats') else self.status
        return entry


@pytest.fixture
def stub(monkeypatch):
    lib = StubLibrary()
    monkeypatch.setattr(_hip, '_lib', lib)
    return lib


def last(stub, name):
    got, args = stub.calls[-1]
    assert got == name and len(args) == len(_hip.SIGNATURES[name][1])
    return args


def _bits(alpha):
    return ctypes.c_uint32.from_buffer_copy(ctypes.c_float(alpha)).value


def _int32(v):
    return ctypes.c_int32(v & 0xffffffff).value


def test_pointers_and_stream(stub, monkeypatch):
    t = torch.zeros(4)
    assert (_hip._ptr(None), _hip._ptr(0x1000), _hip._ptr(t)) == (0, 0x1000, t.data_ptr())
    _hip.coherence(t, 5, 6, 2, None, stream=STREAM)
    assert last(stub, 'gccnmf_coherence') == (t.data_ptr(), 5, 6, 2, 0, STREAM)
    monkeypatch.setattr(_hip, '_stream', lambda device=None: 99)              # no stream given: torch's current one
    _hip.magnitude(0x10, 5, 6, 2, 0x20)
    assert last(stub, 'gccnmf_magnitude') == (0x10, 5, 6, 2, 0x20, 99)


@pytest.mark.parametrize('D,batch,alpha', [(128, 64, 2.0), (3, 1, 0.5), (4096, 65535, 8.0), (200, 5, 0.3)])
def test_angular_spectrogram_words(stub, D, batch, alpha):
    _hip.angular_spectrogram(1, 2, 513, 40, D, batch, 3, 4, stream=STREAM)
    assert last(stub, 'gccnmf_angular_spectrogram') == (1, 2, 513, 40, D, batch, 3, 4, STREAM)
    _hip.angular_spectrogram(1, 2, 513, 40, D, batch, 3, None, nl_alpha=alpha, stream=STREAM)
    args = last(stub, 'gccnmf_angular_spectrogram')
    assert (args[4], args[5]) == _hip.angular_nl_words(D, batch, alpha)
    # GCCNMF_ANGULAR_NL_D / GCCNMF_ANGULAR_NL_BATCH of include/gccnmf_hip.h, evaluated here
    assert args[4] == _int32(D | (_bits(alpha) & 0xffff0000)) and args[5] == _int32(batch | (_bits(alpha) << 16))
    assert args[:4] + args[6:] == (1, 2, 513, 40, 3, 0, STREAM)


def test_peaks_and_tracks_words(stub):
    _hip.pick_tdoa_peaks(1, 128, 192, 3, 8, 2, 3, stream=STREAM)
    assert last(stub, 'gccnmf_pick_tdoa_peaks') == (1, 128, 192, 3, 8, 2, 3, STREAM)
    for T, L in ((50, 9), (50, 99), (50, 100), (7, 1000), (1, 1)):
        _hip.pick_tdoa_tracks(1, 128, T, 3, L, 8, 2, 3, stream=STREAM)
        assert last(stub, 'gccnmf_pick_tdoa_peaks') == (1, 128, T, 3 | 0x100 | min(L, 2 * T - 1) << 9, 8, 2, 3, STREAM)    # T rides in the Dp slot
        assert last(stub, 'gccnmf_pick_tdoa_peaks')[3] == _hip.peaks_tracks_word(3, L, T)


def test_scores_word(stub):
    for tracks, S in ((False, 3), (True, 3 | 0x100)):
        _hip.target_scores_masks(1, 2, 3, 4, 513, 40, 16, 128, 3, 8, 5, 6, None, tracks=tracks, stream=STREAM)
        assert last(stub, 'gccnmf_target_scores_masks') == (1, 2, 3, 4, 513, 40, 16, 128, S, 8, 5, 6, 0, STREAM)
    assert _hip.GCCNMF_SCORES_TRACKS == 0x100


@pytest.mark.parametrize('mode,S,batch,workspace', [('direct', 3, 8, 0x70), ('ratio', 3 | 0x100, 8, 0), ('spatial', 3 | 0x100, 8 | 0x10000, 0x70)])
def test_reconstruct_words(stub, mode, S, batch, workspace):
    _hip.reconstruct(1, 2, 3, None, 5, 6, 513, 40, 16, 3, 8, 0x80, mode=mode, workspace=None if mode == 'ratio' else 0x70, stream=STREAM)
    assert last(stub, 'gccnmf_reconstruct') == (1, 2, 3, 0, 5, 6, 513, 40, 16, S, batch, workspace, 0x80, STREAM)


def test_reconstruct_checks_come_before_the_library(stub):
    with pytest.raises(ValueError):
        _hip.reconstruct(1, 2, 3, None, 5, 6, 513, 40, 16, 3, 8, 0x80, mode='spatial', stream=STREAM)
    with pytest.raises(ValueError):
        _hip.reconstruct(1, 2, 3, None, 5, 6, 513, 40, 16, 3, 65536, 0x80, mode='spatial', workspace=0x70, stream=STREAM)
    with pytest.raises(ValueError):
        _hip.reconstruct(1, 2, 3, None, 5, 6, 513, 40, 16, 3, 8, 0x80, mode='wiener', workspace=0x70, stream=STREAM)
    assert stub.calls == []


def test_reconstruct_workspace_floats(stub):
    assert _hip.reconstruct_workspace_floats('ratio', 40, 16, 3, 8, 528) == 0 and stub.calls == []
    assert _hip.reconstruct_workspace_floats('spatial', 40, 16, 3, 8, 528) == 4 * 8 * 3 * 528 and stub.calls == []
    assert _hip.reconstruct_workspace_floats('spatial', 40, 16, 3, 8, 528) == _hip.reconstruct_spatial_workspace_floats(8, 3, 528)
    assert _hip.reconstruct_workspace_floats('direct', 40, 16, 3, 8, 528) == 4321
    assert stub.calls == [('gccnmf_reconstruct_workspace_floats', (40, 16, 3, 8))]


def test_klnmf_flags(stub):
    def flags(**kw):
        _hip.klnmf(1, 2, 3, 4, 513, 80, 16, 8, 100, 0.5, 1e-16, stream=STREAM, **kw)
        args = last(stub, 'gccnmf_klnmf')
        assert args[:11] + args[12:] == (1, 2, 3, 4, 513, 80, 16, 8, 100, 0.5, 1e-16, STREAM)
        return args[11]
    assert flags() == 0 and flags(flags=3) == 3 and flags(groups=1, flags=2) == 2
    assert flags(groups=2) == 4 | 2 << 8 and flags(groups=2, flags=1) == 1 | 4 | 2 << 8 and flags(groups=4) == 4 | 4 << 8
    assert flags(fixed_w=True) == 1 << 16 == _hip.GCCNMF_FLAG_FIXED_W
    assert flags(fixed_w=True, h_ones=True) == (1 << 16) | (1 << 17) == _hip.GCCNMF_FLAG_FIXED_W | _hip.GCCNMF_FLAG_H_ONES


def test_klnmf_divergence_and_chain_status(stub):
    F, N, K, batch = 33, 70, 5, 3
    Fp, Np = 48, 128
    ws = torch.arange(batch * Fp * Np + 2 * batch + 8, dtype=torch.float32)
    for fixed, flags in ((False, 0), (True, 1 << 16)):
        d = _hip.klnmf_divergence(1, 2, 3, ws, F, N, K, batch, fixed=fixed, stream=STREAM)
        assert last(stub, 'gccnmf_klnmf_stage') == (1, 2, 3, ws.data_ptr(), F, N, K, batch, 0.0, 0.0, flags, 7, STREAM)
        assert d.dtype == torch.float64 and d.shape == (batch,) and d.data_ptr() == ws.data_ptr() + 4 * batch * Fp * Np
    stub.chain_word = 2
    assert _hip.klnmf_chain_status(0x40, F, N, K, batch) == 2
    assert stub.calls[-1][0] == 'gccnmf_klnmf_chain_status' and stub.calls[-1][1][:5] == (0x40, F, N, K, batch)


def test_thin_wrappers_keep_the_header_order(stub):
    _hip.stft_stereo(1, 16000, 1024, 256, 59, 4, 2, 3, 4, 5, 6, stream=STREAM)
    assert last(stub, 'gccnmf_stft_stereo') == (1, 32000, 16000, 1024, 256, 59, 4, 2, 3, 4, 5, 6, STREAM)
    _hip.stft_stereo(1, 16000, 1024, 256, 59, 4, 2, 3, 4, 5, None, pcm16=True, stream=STREAM)
    assert last(stub, 'gccnmf_stft_stereo_pcm16') == (1, 16000, 16000, 1024, 256, 59, 4, 2, 3, 4, 5, 0, STREAM)
    for center, frames in ((True, None), (False, 9)):
        _hip.istft_ola(1, 6, 1024, 256, 59, 4, 2, 3, 0.5, center, frames, 8, stream=STREAM)
        assert last(stub, 'gccnmf_istft_ola') == (1, 6, 1024, 256, 59, 4, 2, 3, 0.5, int(center), frames or 0, 8, STREAM)
    _hip.ola_frames_halo(None, 0, 2, 6, 1024, 256, 59, 768, 15000, 0.5, 7, stream=STREAM)
    assert last(stub, 'gccnmf_ola_frames_halo') == (0, 0, 2, 6, 1024, 256, 59, 768, 15000, 0.5, 7, STREAM)
    _hip.pack_pcm16(1, 12, 14848, 2, 3, stream=STREAM)
    assert last(stub, 'gccnmf_pack_pcm16') == (1, 12, 14848, 2, 3, STREAM)
    _hip.argmax_targets(1, 16, 59, 3, 4, 2, stream=STREAM)
    assert last(stub, 'gccnmf_argmax_targets') == (1, 16, 59, 3, 4, 2, STREAM)


RT_POINTERS = tuple(range(0x100, 0x100 + 23))               # block_in .. Rv as raw addresses
RT_GEOMETRY = (512, 64, 64, 256, 256, 64, 64, 128)          # windowSize, hopSize, blockSize, K, Kp, D, Dp, numTDOAHistory
BANK, MULTI, ROW8 = 8, 1 << 20, 1 << 24                     # frames_mode_bits of include/gccnmf_hip.h


def rt_call(target_mode=_hip.TARGET_MODE_WINDOW_FUNCTION, **mode):
    _hip.rt_process_block(*RT_POINTERS, *RT_GEOMETRY, target_mode, True, False, 6, 3, 1, stream=STREAM, **mode)


@pytest.mark.parametrize('mode,word', [
    ({}, 0), (dict(frames=True), 1), (dict(localize='skip'), 2), (dict(localize='only'), 4), (dict(frames=True, localize='only'), 5),
    (dict(streams=1), BANK), (dict(streams=3), BANK | 2 << 8), (dict(streams=4096), BANK | 4095 << 8),
    (dict(targets=1), MULTI), (dict(targets=8), MULTI | 7 << 21),
    (dict(streams=3, targets=2, localize='skip'), 2 | BANK | 2 << 8 | MULTI | 1 << 21), (dict(nl_row=True), ROW8)],
    ids=lambda v: ' '.join('%s=%s' % kv for kv in v.items()) or 'plain' if isinstance(v, dict) else None)
def test_rt_process_block_word(stub, mode, word):
    target_mode = _hip.TARGET_MODE_MULTIPLE if 'targets' in mode else _hip.TARGET_MODE_WINDOW_FUNCTION
    rt_call(target_mode, **mode)
    args = last(stub, 'gccnmf_rt_process_block_ll')
    assert args[35] == word == _hip.rt_mode_word(**mode)
    # every other argument in the header's order (the switches as 0 / 1), the stream last
    assert args[:35] + args[36:] == RT_POINTERS + RT_GEOMETRY + (target_mode, 1, 0, 6, 3, 1, STREAM)


def test_rt_process_block_defaults_and_pointers(stub, monkeypatch):
    t = torch.zeros(4)
    monkeypatch.setattr(_hip, '_stream', lambda device=None: 99)              # no stream given: torch's current one
    _hip.rt_process_block(None, t, *RT_POINTERS[2:], *RT_GEOMETRY, 0, 0, 1, 6)
    args = last(stub, 'gccnmf_rt_process_block_ll')
    assert args[:2] == (0, t.data_ptr()) and args[31:] == (0, 0, 1, 6, 0, 0, 2, 99)      # numHUpdates 0, the reference's hand-out of 2
    assert (_hip.MAX_BANK_STREAMS, _hip.MAX_SOURCES, _hip.RT_BANK_LAYOUT, _hip.RT_MULTI_LAYOUT, _hip.RT_ROW8_LAYOUT) == (4096, 8, BANK, MULTI, ROW8)
    assert (_hip.RT_FRAMES, _hip.RT_SKIP_LOCALIZE, _hip.RT_ONLY_LOCALIZE) == (1, 2, 4)


@pytest.mark.parametrize('mode', [
    dict(streams=2, frames=True), dict(nl_row=True, streams=2), dict(nl_row=True, targets=2), dict(nl_row=True, streams=2, targets=2),
    dict(targets=2, target_mode=_hip.TARGET_MODE_WINDOW_FUNCTION), dict(targets=2, target_mode=_hip.TARGET_MODE_BOXCAR),
    dict(streams=0), dict(streams=4097), dict(streams=-1), dict(targets=0), dict(targets=9), dict(localize='never'), dict(localize=4)],
    ids=lambda v: ' '.join('%s=%s' % kv for kv in v.items()))
def test_rt_process_block_checks_come_before_the_library(stub, mode):
    mode = dict(mode)
    target_mode = mode.pop('target_mode', _hip.TARGET_MODE_MULTIPLE)
    with pytest.raises(ValueError):
        rt_call(target_mode, **mode)
    assert stub.calls == []


STAGES = [
    ('gccnmf_stft_stereo', lambda: _hip.stft_stereo(1, 16000, 1024, 256, 59, 4, 2, 3, 4, 5, 6, stream=STREAM)),
    ('gccnmf_stft_stereo_pcm16', lambda: _hip.stft_stereo(1, 16000, 1024, 256, 59, 4, 2, 3, 4, 5, 6, pcm16=True, stream=STREAM)),
    ('gccnmf_istft_ola', lambda: _hip.istft_ola(1, 6, 1024, 256, 59, 4, 2, 3, 0.5, True, None, 8, stream=STREAM)),
    ('gccnmf_ola_frames_halo', lambda: _hip.ola_frames_halo(None, 0, 2, 6, 1024, 256, 59, 768, 15000, 0.5, 7, stream=STREAM)),
    ('gccnmf_pack_pcm16', lambda: _hip.pack_pcm16(1, 12, 14848, 2, 3, stream=STREAM)),
    ('gccnmf_coherence', lambda: _hip.coherence(1, 513, 59, 1, 2, stream=STREAM)),
    ('gccnmf_magnitude', lambda: _hip.magnitude(1, 513, 59, 1, 2, stream=STREAM)),
    ('gccnmf_klnmf', lambda: _hip.klnmf(1, 2, 3, 4, 513, 80, 16, 8, 100, 0.0, 1e-16, stream=STREAM)),
    ('gccnmf_klnmf_stage (divergence)', lambda: _hip.klnmf_divergence(1, 2, 3, torch.zeros(8), 5, 6, 2, 1, stream=STREAM)),
    ('gccnmf_klnmf_chain_status', lambda: _hip.klnmf_chain_status(1, 513, 80, 16, 8)),
    ('gccnmf_angular_spectrogram', lambda: _hip.angular_spectrogram(1, 2, 513, 40, 128, 8, 3, 4, nl_alpha=2.0, stream=STREAM)),
    ('gccnmf_pick_tdoa_peaks', lambda: _hip.pick_tdoa_peaks(1, 128, 192, 3, 8, 2, 3, stream=STREAM)),
    ('gccnmf_pick_tdoa_peaks (tracks)', lambda: _hip.pick_tdoa_tracks(1, 128, 50, 3, 9, 8, 2, 3, stream=STREAM)),
    ('gccnmf_target_scores_masks', lambda: _hip.target_scores_masks(1, 2, 3, 4, 513, 40, 16, 128, 3, 8, 5, 6, 7, stream=STREAM)),
    ('gccnmf_argmax_targets', lambda: _hip.argmax_targets(1, 16, 59, 3, 4, 2, stream=STREAM)),
    ('gccnmf_reconstruct', lambda: _hip.reconstruct(1, 2, 3, None, 5, 6, 513, 40, 16, 3, 8, 9, mode='ratio', stream=STREAM)),
    ('gccnmf_rt_process_block_ll', lambda: rt_call(localize='skip')),
]


@pytest.mark.parametrize('what,call', STAGES, ids=[s[0] for s in STAGES])
def test_a_status_raises_with_the_name_of_the_stage(stub, what, call):
    call()                                                   # status 0: no exception
    stub.status = 2
    with pytest.raises(_hip.HipLibraryError) as e:
        call()
    assert str(e.value) == '%s failed: GCCNMF_ERR_LAUNCH (HIP launch failed)' % what
