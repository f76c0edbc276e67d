"""CPU: every argument error of the entry points of csrc/fft.hip is decided before any HIP call, so it is testable without a device:
a rejected call returns GCCNMF_ERR_ARG (1) or GCCNMF_ERR_UNSUPPORTED (3); one that reached a launch or a HIP query here would return
GCCNMF_ERR_LAUNCH (2).  Pointers are the address 4096: nothing may dereference them.  Every call below MUST be one the library rejects."""
import pytest

ARG, LAUNCH, UNSUPPORTED = 1, 2, 3
P = 4096


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def stft_args(x=P, stride=100000, n=40000, n_fft=1024, hop=256, T=8, batch=2, window=P, twiddle=P, X=P, V=P, CC=P):
    return (x, stride, n, n_fft, hop, T, batch, window, twiddle, X, V, CC, None)


@pytest.mark.parametrize('entry', ['gccnmf_stft_stereo', 'gccnmf_stft_stereo_pcm16'])
def test_forward_transform_rejections(lib, entry):
    fn = getattr(lib, entry)
    for bad in (dict(n_fft=32), dict(n_fft=8192), dict(n_fft=1000), dict(n_fft=1023), dict(n_fft=0), dict(n_fft=-1024),
                dict(hop=0), dict(hop=-1), dict(T=0), dict(batch=0),
                dict(n=(8 - 1) * 256 + 1024 - 1),                       # one sample short of (T - 1) hop + n_fft
                dict(n=1023, T=1), dict(n=4095, n_fft=4096, T=1),
                dict(x=0), dict(window=0), dict(twiddle=0), dict(X=0)):
        assert fn(*stft_args(**bad)) == ARG, bad


def istft_args(spec=P, nsig=2, n_fft=1024, hop=256, T=8, batch=1, window=P, twiddle=P, gain=1.0, center=1, frames=P, y=P):
    return (spec, nsig, n_fft, hop, T, batch, window, twiddle, gain, center, frames, y, None)


@pytest.mark.parametrize('frames', [P, 0], ids=['two-kernel', 'fused'])
def test_inverse_transform_rejections(lib, frames):
    fn = lib.gccnmf_istft_ola
    for bad in (dict(n_fft=32), dict(n_fft=8192), dict(n_fft=1000), dict(hop=0), dict(T=0), dict(batch=0),
                dict(nsig=0), dict(nsig=1), dict(nsig=3), dict(nsig=-2),
                dict(T=1, center=1),                                    # L = n_fft - n_fft < 1: in BOTH forms before the first launch
                dict(T=1, center=1, n_fft=64, hop=16), dict(T=1, center=1, n_fft=4096, hop=4096),
                dict(spec=0), dict(window=0), dict(twiddle=0), dict(y=0)):
        assert fn(*istft_args(frames=frames, **bad)) == ARG, bad


def test_fused_inverse_transform_is_unsupported_by_rule(lib):
    """frames = NULL: n_fft + 3 hop > 2048 (the sliding accumulator's 8 x 256 positions), and hop > n_fft (samples between the frames
    that no frame touches, which the fused pass would leave unwritten) -> GCCNMF_ERR_UNSUPPORTED, nothing launched."""
    fn = lib.gccnmf_istft_ola
    for n_fft, hop in ((1024, 342), (1024, 512), (1024, 1024), (2048, 1), (2048, 256), (4096, 512), (512, 513), (64, 662),
                       (256, 300), (64, 65), (256, 257), (512, 600)):
        for T in (1, 6, 33):
            assert fn(*istft_args(n_fft=n_fft, hop=hop, T=T, center=0, frames=0)) == UNSUPPORTED, (n_fft, hop, T)
    # (the argument errors win over the rule)
    assert fn(*istft_args(n_fft=256, hop=300, T=1, center=1, frames=0)) == ARG
    assert fn(*istft_args(n_fft=256, hop=300, T=6, nsig=3, frames=0)) == ARG


def halo_args(prev=P, halo=3, frames=P, nsig=6, n_fft=1024, hop=256, T=10, first=0, L=1000, gain=1.0, y=P):
    return (prev, halo, frames, nsig, n_fft, hop, T, first, L, gain, y, None)


def test_ola_frames_halo_rejections(lib):
    fn = lib.gccnmf_ola_frames_halo
    stream = 1024 + 256 * (3 + 10 - 1)                                   # n_fft + hop (halo + T - 1) samples in the overlap-added stream
    for bad in (dict(prev=0), dict(halo=-1), dict(frames=0), dict(y=0), dict(nsig=0), dict(n_fft=1), dict(hop=0), dict(T=0),
                dict(first=-1), dict(L=0), dict(L=-5),
                dict(first=0, L=stream + 1), dict(first=1, L=stream), dict(first=stream, L=1),      # the range rule: first + L <= stream
                dict(halo=0, prev=0, first=0, L=1024 + 256 * 9 + 1)):
        assert fn(*halo_args(**bad)) == ARG, bad


def test_pack_pcm16_rejections(lib):
    fn = lib.gccnmf_pack_pcm16
    for args in ((P, 0, 100, P, P), (P, 3, 0, P, P), (P, -1, 100, P, P), (P, 3, -1, P, P), (0, 3, 100, P, P), (P, 3, 100, 0, P), (P, 3, 100, P, 0)):
        assert fn(*args, None) == ARG, args


def test_any_size_transform_rejections(lib):
    f = lib.gccnmf_stft_dft          # (x, x_stride, n_samples, n_fft, hop, T, nsig, basis, workspace, X, stream)
    for args in ((P, 9000, 9000, 1, 250, 4, 2, P, P, P), (P, 9000, 9000, 8193, 250, 1, 2, P, P, P), (P, 9000, 9000, 1000, 0, 4, 2, P, P, P),
                 (P, 9000, 9000, 1000, 250, 0, 2, P, P, P), (P, 9000, 9000, 1000, 250, 4, 0, P, P, P),
                 (P, 9000, 3 * 250 + 1000 - 1, 1000, 250, 4, 2, P, P, P),                          # one sample short
                 (0, 9000, 9000, 1000, 250, 4, 2, P, P, P), (P, 9000, 9000, 1000, 250, 4, 2, 0, P, P), (P, 9000, 9000, 1000, 250, 4, 2, P, 0, P),
                 (P, 9000, 9000, 1000, 250, 4, 2, P, P, 0)):
        assert f(*args, None) == ARG, args
    g = lib.gccnmf_istft_dft         # (spec, nsig, n_fft, hop, T, ibasis, gain, center, workspace, y, stream)
    for args in ((P, 2, 375, 125, 4, P, 1.0, 0, P, P), (P, 2, 1001, 250, 4, P, 1.0, 1, P, P),       # odd n_fft
                 (P, 2, 0, 250, 4, P, 1.0, 0, P, P), (P, 2, 8194, 250, 4, P, 1.0, 0, P, P), (P, 2, 1000, 0, 4, P, 1.0, 0, P, P),
                 (P, 2, 1000, 250, 0, P, 1.0, 0, P, P), (P, 0, 1000, 250, 4, P, 1.0, 0, P, P),
                 (P, 2, 1000, 250, 1, P, 1.0, 1, P, P),                                              # L < 1
                 (0, 2, 1000, 250, 4, P, 1.0, 0, P, P), (P, 2, 1000, 250, 4, 0, 1.0, 0, P, P), (P, 2, 1000, 250, 4, P, 1.0, 0, 0, P),
                 (P, 2, 1000, 250, 4, P, 1.0, 0, P, 0)):
        assert g(*args, None) == ARG, args
    assert lib.gccnmf_dft_workspace_floats(1, 4, 2) == -1 and lib.gccnmf_dft_workspace_floats(1000, 0, 2) == -1 and lib.gccnmf_dft_workspace_floats(1000, 4, 0) == -1
