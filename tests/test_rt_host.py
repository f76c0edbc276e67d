"""CPU: every argument check of gccnmf_rt_process_block_ll (csrc/rt.hip) is decided before any HIP call, so it is testable without a
device: a rejected call returns GCCNMF_ERR_ARG (1) or GCCNMF_ERR_UNSUPPORTED (3); one that reached a launch or a HIP query here would
return GCCNMF_ERR_LAUNCH (2).  Pointers are the address 4096: nothing may dereference them.  Every call below MUST be one the library
rejects; one rejection per clause of the launcher's checks."""
import pytest

ARG, LAUNCH, UNSUPPORTED = 1, 2, 3
P = 4096
POINTERS = ('block_in', 'block_out', 'in_ring', 'out_ring', 'X', 'Y', 'C', 'HMask', 'argmaxTDOA', 'tfMask', 'hist', 'hist_pos', 'target', 'gccphat',
            'W', 'cosT', 'sinT', 'window', 'synthesis_window', 'twiddle', 'colsumW', 'Hcoef', 'Rv')
INTS = dict(windowSize=1024, hopSize=256, blockSize=512, K=100, Kp=128, D=33, Dp=64, numTDOAHistory=16, target_mode=2, separation_enabled=1,
            localization_enabled=1, localization_window=6, frames_mode=0, numHUpdates=0, out_delay_blocks=2)
BANK, MULTI, ROW8 = 8, 1 << 20, 1 << 24


@pytest.fixture(scope='module')
def call():
    from gcc_nmf_amd import _hip
    fn = _hip.lib().gccnmf_rt_process_block_ll

    def call(**kw):
        ptrs = [kw.pop(k, P) for k in POINTERS]
        ints = dict(INTS)
        for k in list(kw):
            assert k in ints, k
            ints[k] = kw.pop(k)
        return fn(*ptrs, *[ints[k] for k in INTS], None)
    return call


def test_the_frames_mode_word(call):
    for bits in (1 << 25, 1 << 30, -1 << 25,                     # a bit above 24
                 BANK | 1,                                       # the bank layout in frames mode
                 2 << 8, 1 | (1 << 8),                           # stream-count bits without the bank layout
                 ROW8 | BANK, ROW8 | MULTI):                     # the 8-word single-stream row in a layout that always has it
        assert call(frames_mode=bits, target_mode=1 if bits & MULTI else 2) == ARG, hex(bits)
    assert call(frames_mode=MULTI, target_mode=2) == ARG and call(frames_mode=MULTI | (2 << 21), target_mode=0) == ARG     # multi needs mode 1
    assert call(frames_mode=1 << 21, target_mode=1) == ARG and call(frames_mode=7 << 21) == ARG                             # target bits alone


@pytest.mark.parametrize('name', [p for p in POINTERS if p not in ('argmaxTDOA', 'gccphat', 'colsumW', 'Hcoef', 'Rv')])
def test_a_null_pointer(call, name):
    assert call(**{name: 0}) == ARG
    if name not in ('block_in', 'block_out'):                    # (frames mode has no block buffers; the others stay required)
        assert call(frames_mode=1, **{name: 0}) == ARG
    assert call(frames_mode=4, **{name: 0}) == ARG               # the localisation-only call checks the same list first


def test_the_inference_buffers_and_the_delay(call):
    assert call(numHUpdates=-1) == ARG
    for name in ('colsumW', 'Hcoef', 'Rv'):
        assert call(numHUpdates=1, **{name: 0}) == ARG and call(numHUpdates=3, frames_mode=1, **{name: 0}) == ARG
    for od in (0, 8, -1, 100):
        assert call(out_delay_blocks=od) == ARG


def test_the_sizes(call):
    for bad in (dict(windowSize=2), dict(windowSize=0), dict(windowSize=-1024), dict(windowSize=4098), dict(windowSize=8192),
                dict(windowSize=1023), dict(windowSize=401), dict(windowSize=5),
                dict(hopSize=0), dict(hopSize=-256),
                dict(blockSize=255), dict(blockSize=0),                          # blockSize < hopSize
                dict(blockSize=600), dict(blockSize=257),                        # not a multiple of the hop
                dict(K=0), dict(K=-1), dict(Kp=100), dict(Kp=96), dict(Kp=64), dict(Kp=0), dict(K=129),      # Kp % 64, Kp < K
                dict(D=0), dict(D=-3), dict(D=1025, Dp=1056), dict(Dp=33), dict(Dp=48), dict(Dp=32), dict(Dp=0),
                dict(numTDOAHistory=0), dict(numTDOAHistory=-4), dict(localization_window=0), dict(localization_window=-1),
                dict(localization_window=17), dict(numTDOAHistory=5)):           # window > history
        assert call(**bad) == ARG, bad
        assert call(frames_mode=1, **bad) == ARG, bad


def test_a_block_too_short_for_its_windows_is_unsupported_by_rule(call):
    """Streaming: 8 * blockSize < windowSize + (Tc - 1) hopSize -> GCCNMF_ERR_UNSUPPORTED, nothing launched; frames mode has no such rule,
    and the argument errors win over it."""
    for N, hop, B in ((1024, 64, 64), (1024, 127, 127), (4096, 256, 256), (4096, 511, 511), (4094, 100, 500), (64, 1, 7), (400, 7, 49)):
        assert 8 * B < N + (B // hop - 1) * hop
        for bits in (0, 2, 4, BANK | (4 << 8)):
            assert call(windowSize=N, hopSize=hop, blockSize=B, frames_mode=bits) == UNSUPPORTED, (N, hop, B, bits)
        assert call(windowSize=N, hopSize=hop, blockSize=B, out_delay_blocks=0) == ARG
        assert call(windowSize=N, hopSize=hop, blockSize=B, X=0) == ARG
