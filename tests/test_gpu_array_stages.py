"""-m gpu: the two entry points of libgccnmf_array.so (include/gccnmf_array.h, csrc/array.hip) through the C ABI.

gccnmf_array_features: block p of CC is, bit for bit, gccnmf_coherence of the stereo spectrogram made of channels (a, b) of pair p; V is,
bit for bit, gccnmf_magnitude of each channel; every padding element is written as zero; a file alone gives the bits it gives in a batch.

gccnmf_array_reconstruct: plane (i, c) is, bit for bit, plane (i, 0) of gccnmf_reconstruct in ratio mode on the stereo problem whose
channel 0 is channel c.  Both libraries instantiate the one kernel of csrc/ratio_kernel.h, so this checks its M / nsig_pitch / c T
addressing -- the (file, channel) of a workgroup, the columns of H_c, the slot i M + c of a plane -- at M channels against M = 2, not that
two kernels agree.  And it is within gcc_checks.check_gemm_like(Kd = K) of the float64 restatement tests/array_restatement.py, relative
to |X|: num_i and den are chains of at most K fma of non-negative terms (relative error <= K u each, no cancellation; the soft form's
mask products add one rounding per term, the one-hot form's S - 1 additions of den replace as many fma that a masked-out term makes
exact), num_i <= den, one quotient and one product: at most (2 K + 4) u |X| <= 2 (K + 4) u |X|, the bound of check_gemm_like with
absprod = |X|.  A NaN planted in W must come out as NaN exactly where the restatement has NaN.  The stereo planes of the bit comparison
meet the same bound themselves, so that the separation library's instantiations for 4 to 7 targets are checked against a reference too.

Every channel count 2 ... 8 (pair indexes up to 27) and every target count 1 ... 8 runs, the latter in both forms; CASES says which row tile
shapes of the reconstruction (128 rows a tile, the last row of F = 32 n + 1 on the VALU) each F stands for."""
import numpy as np
import pytest

import array_restatement as A
import gcc_checks as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

OK, ARG, UNSUPPORTED = 0, 1, 3
NAN = float('nan')


@pytest.fixture(scope='module')
def libs():
    from gcc_nmf_amd import _array, _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib(), _array.lib()


def rup(a, b):
    return -(-a // b) * b


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


def padded_X(X, Fp, Tp, fill=NAN):
    """(B, M, F, T) complex64 -> [B][M][Fp][Tp][2] float32 with `fill` in the padding (the kernels read no padding of X)."""
    B, M, F, T = X.shape
    Xp = np.full((B, M, Fp, Tp, 2), fill, np.float32)
    Xp[:, :, :F, :T, 0], Xp[:, :, :F, :T, 1] = X.real, X.imag
    return Xp


# ---- features ---------------------------------------------------------------------------------------------------------------------------------
def feature_spectra(B, M, F, T, seed):
    rng = np.random.RandomState(seed)
    X = (rng.randn(B, M, F, T) + 1j * rng.randn(B, M, F, T)).astype(np.complex64)
    X[:, 0, 1, 0] = 0                                   # exactly zero in one channel
    X[:, :, F - 1, T - 1] = 0                           # ... in all channels
    X[B - 1, M - 1, 5, :] = 0
    X[0, 0, 7, 1] = np.complex64(1e-30 + 0j)            # tiny but not zero: keeps its phase
    return X


def features_case(M, T, F):
    from gcc_nmf_amd import _array, _hip
    B, Fp = 3, rup(F, 16)
    Tp, Np, Np2, P = rup(T, 64), rup(M * T, 64), rup(2 * T, 64), M * (M - 1) // 2
    assert len(A.pairs(M)) == P
    X = feature_spectra(B, M, F, T, 10 * M + T)
    dX = dev(padded_X(X, Fp, Tp))
    V = torch.full((B, Fp, Np), NAN, dtype=torch.float32, device='cuda')
    CC = torch.full((B, 2, P * Fp, Tp), NAN, dtype=torch.float32, device='cuda')
    _array.features(dX, M, F, T, B, V, CC)
    torch.cuda.synchronize()
    C.check_written(V.cpu().numpy(), 'V')
    C.check_written(CC.cpu().numpy(), 'CC')
    blocks = CC.view(B, 2, P, Fp, Tp)
    C.check_zero(blocks[:, :, :, F:, :].cpu().numpy(), 'CC rows >= F of every pair')
    C.check_zero(blocks[:, :, :, :, T:].cpu().numpy(), 'CC frames >= T')
    C.check_zero(V[:, F:, :].cpu().numpy(), 'V rows >= F')
    C.check_zero(V[:, :, M * T:].cpu().numpy(), 'V columns >= M T')
    wrong = []
    for p, (a, b) in enumerate(A.pairs(M)):
        Xs = dX[:, [a, b]].contiguous()
        CCs = torch.zeros((B, 2, Fp, Tp), dtype=torch.float32, device='cuda')
        _hip.coherence(Xs, F, T, B, CCs)
        if not same_bits(blocks[:, :, p, :F, :T], CCs[:, :, :F, :T]):
            wrong.append((p, (a, b)))
    assert not wrong, 'blocks that are not gccnmf_coherence of their pair, as (p, (a, b)): %s' % wrong
    c = blocks[:, :, :, :F, :T].cpu().numpy()
    assert (c[:, :, :, F - 1, T - 1] == 0).all() and (c[:, :, :M - 1, 1, 0] == 0).all(), 'a zero magnitude gives (0, 0)'
    assert np.abs(np.hypot(c[0, 0, 0, 7, 1], c[0, 1, 0, 7, 1]) - 1) < 1e-5, 'a tiny bin keeps its phase'
    for ch in range(M):
        Xs = dX[:, [ch, ch]].contiguous()
        Vs = torch.zeros((B, Fp, Np2), dtype=torch.float32, device='cuda')
        _hip.magnitude(Xs, F, T, B, Vs)
        assert same_bits(V[:, :F, ch * T:(ch + 1) * T], Vs[:, :F, :T]), 'channel %d' % ch
    # either output alone; a file alone
    V1 = torch.full_like(V, NAN)
    C1 = torch.full_like(CC, NAN)
    _array.features(dX, M, F, T, B, V1, None)
    _array.features(dX, M, F, T, B, None, C1)
    assert same_bits(V1, V) and same_bits(C1, CC)
    Va = torch.full((1, Fp, Np), NAN, dtype=torch.float32, device='cuda')
    Ca = torch.full((1, 2, P * Fp, Tp), NAN, dtype=torch.float32, device='cuda')
    _array.features(dX[1:2].contiguous(), M, F, T, 1, Va, Ca)
    assert same_bits(Va[0], V[1]) and same_bits(Ca[0], CC[1]), 'a file alone gives the bits it gives in the batch'
    ref_V, ref_C = A.features(X[1])
    assert np.abs(V[1, :F, :M * T].cpu().numpy() - ref_V).max() <= 4 * 2.0 ** -24 * np.abs(ref_V).max()


@pytest.mark.parametrize('T', [2, 64, 67])
@pytest.mark.parametrize('M', [2, 3, 4, 5, 6, 7, 8])
def test_features_are_the_stereo_kernels_per_pair_and_channel(libs, M, T):
    """F = 33: fifteen padding rows (Fp - F = 15) between the pair blocks."""
    features_case(M, T, 33)


@pytest.mark.parametrize('M,T,F', [(8, 67, 48), (3, 2, 32)])
def test_features_without_padding_rows_between_the_pairs(libs, M, T, F):
    """F = Fp: pair p + 1 starts in the row after pair p's last bin."""
    assert F % 16 == 0
    features_case(M, T, F)


# ---- reconstruction ---------------------------------------------------------------------------------------------------------------------------
def problem(B, M, F, T, K, S, seed):
    """float32 operands as tests/test_gpu_ratio_reconstruction.py builds them (W's last row and last atom x 100), per file; file 0 has a
    column of H that is all zero in channel M - 1 (den = 0), the last file a NaN in one element of W."""
    rng = np.random.RandomState(seed)
    X = (rng.uniform(0.5, 2.0, (B, M, F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (B, M, F, T)))).astype(np.complex64)
    W = rng.uniform(0.01, 1.0, (B, F, K)).astype(np.float32)
    W[:, F - 1] *= np.float32(100)
    W[:, :, K - 1] *= np.float32(100)
    H = rng.uniform(0.01, 1.0, (B, K, M * T)).astype(np.float32)
    am = rng.randint(0, S, (B, K, T)).astype(np.uint8)
    masks = rng.uniform(0.0, 1.0, (B, S, K, T)).astype(np.float32)
    H[0, :, (M - 1) * T + T // 2] = 0
    W[B - 1, F // 2, K // 2] = np.nan
    return X, W, H, am, masks


def device_operands(X, W, H, am, masks, nsig_pitch):
    B, M, F, T = X.shape
    K, S = W.shape[2], masks.shape[1]
    Fp, Kp, Tp, Np = rup(F, 16), rup(K, 64), rup(T, 64), rup(M * T, 64)
    Wp = np.zeros((B, Fp, Kp), np.float32)
    Wp[:, :F, :K] = W
    Hp = np.zeros((B, Kp, Np), np.float32)
    Hp[:, :K, :M * T] = H
    Ap = np.zeros((B, Kp, Tp), np.uint8)
    Ap[:, :K, :T] = am
    Mp = np.full((B, S, Kp, Tp), np.float32(7.0))               # the padding of a caller's mask buffer is not the library's: garbage
    Mp[:, :, :K, :T] = masks
    return dev(Wp), dev(Hp), dev(Ap), dev(Mp), dev(padded_X(X, Fp, Tp, 0.0))


def stereo_planes(hip_mod, dW, dH, dA, dM, dX, c, M, F, T, K, S, soft):
    """gccnmf_reconstruct in ratio mode on the stereo problem whose channel 0 is channel c -> [B][S][Fp][Tp][2], its planes (i, 0)."""
    B, Kp = dH.shape[0], dH.shape[1]
    Fp, Tp, Np2 = dX.shape[2], dX.shape[3], rup(2 * T, 64)
    Hs = torch.zeros((B, Kp, Np2), dtype=torch.float32, device='cuda')
    Hs[:, :, :T] = dH[:, :, c * T:(c + 1) * T]
    Hs[:, :, T:2 * T] = dH[:, :, c * T:(c + 1) * T]
    Xs = dX[:, [c, c]].contiguous()
    spec = torch.full((B, 2 * S, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    hip_mod.reconstruct(dW, Hs, None if soft else dA, dM if soft else None, Xs, None, F, T, K, S, B, spec, mode='ratio')
    return spec.view(B, S, 2, Fp, Tp, 2)[:, :, 0]


# (M, F, K, T, S): every M in 2 ... 8, every S in 1 ... 8 (each in both forms), K in 5 / 16 / 70 and T in 3 / 64 / 70 at least once each, and
# every row-tile shape of the reconstruction: F = 33 tail, one tile; 41 no tail, one tile; 129 tail, 128 MFMA rows, exactly one tile; 161 tail,
# 160 MFMA rows, a second tile of 32; 200 no tail, Fp = 208, a partial second tile (the min(row, Fp - 1) clamp); 257 tail, exactly two tiles.
CASES = [(2, 33, 5, 3, 1),         # the smallest of everything
         (3, 41, 16, 64, 2),
         (5, 33, 70, 70, 8),       # both accumulator sets of the tail row in full
         (3, 33, 16, 70, 3),
         (2, 41, 70, 64, 3),
         (5, 41, 5, 3, 2),
         (4, 129, 16, 3, 4),       # S = 4: the first set full, the second unused; one tile exactly
         (6, 161, 5, 64, 5),       # S = 5: one target in the second set; a second tile of 32 rows under a tail
         (7, 200, 70, 3, 6),       # S = 6; the clamp path
         (3, 257, 16, 64, 7),      # S = 7; two full tiles under a tail
         (8, 257, 70, 70, 8)]      # the corner


@pytest.mark.parametrize('soft', [False, True], ids=['one-hot', 'soft'])
@pytest.mark.parametrize('M,F,K,T,S', CASES, ids=['M%d-F%d-K%d-T%d-S%d' % c for c in CASES])
def test_reconstruct_is_the_stereo_kernel_per_channel_and_within_the_float64_bound(libs, M, F, K, T, S, soft):
    from gcc_nmf_amd import _array, _hip
    B = 3
    X, W, H, am, masks = problem(B, M, F, T, K, S, 1000 * M + 10 * K + S)
    pitch = S * M + 1 + (S * M + 1) % 2                          # at least one spare slot, even
    dW, dH, dA, dM, dX = device_operands(X, W, H, am, masks, pitch)
    Fp, Tp = dX.shape[2], dX.shape[3]
    spec = torch.full((B, pitch, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    _array.reconstruct(dW, dH, None if soft else dA, dM if soft else None, dX, M, F, T, K, S, B, pitch, spec)
    torch.cuda.synchronize()
    assert bool(torch.isnan(spec[:, S * M:]).all()), 'slots beyond S M are not touched'
    planes = spec[:, :S * M].view(B, S, M, Fp, Tp, 2)
    C.check_zero(planes[:B - 1, :, :, F:].cpu().numpy(), 'rows >= F')
    C.check_zero(planes[:, :, :, :, T:].cpu().numpy(), 'frames >= T')
    C.check_zero(planes[B - 1, :, :, F:].cpu().numpy(), 'rows >= F of the file with the NaN')
    stereo = torch.empty_like(planes)
    for c in range(M):
        stereo[:, :, c] = stereo_planes(_hip, dW, dH, dA, dM, dX, c, M, F, T, K, S, soft)
        assert same_bits(planes[:, :, c], stereo[:, :, c]), 'channel %d' % c
    got, got_stereo = [(a[..., 0] + 1j * a[..., 1]).astype(np.complex64) for a in (planes[:, :, :, :F, :T].cpu().numpy(),
                                                                                    stereo[:, :, :, :F, :T].cpu().numpy())]
    for b in range(B):
        ref = A.ratio_soft(W[b], H[b], masks[b], X[b]) if soft else A.ratio_one_hot(W[b], H[b], am[b], S, X[b])
        nan = np.isnan(ref)
        assert nan.any() == (b == B - 1)
        if b == B - 1:
            assert nan[:, :, F // 2, :].all() and not np.delete(nan, F // 2, axis=2).any()
        # (the stereo planes are checked on their own, not through the bit comparison above: they are the only float64 check of the
        # separation library's ratio_kernel instantiations at 4 to 7 targets)
        for name, g in (('array', got[b]), ('stereo', got_stereo[b])):
            assert np.array_equal(np.isnan(g), nan), '%s kernel, file %d: NaN exactly where the restatement has NaN' % (name, b)
            C.report_gemm_like(np.where(nan, 0, g), np.where(nan, 0, ref), np.broadcast_to(np.abs(X[b])[None], ref.shape), K,
                               what='%s kernel, file %d' % (name, b))
    assert (got[0, :, M - 1, :, T // 2] == 0).all(), 'den = 0: every target is exactly 0'
    assert (np.abs(got[0, :, M - 1, :, (T // 2 + 1) % T]) > 0).any() or T == 1
    # a file alone, and in another place of the batch
    alone = torch.full((1, pitch, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    one = lambda t: None if t is None else t[1:2].contiguous()
    _array.reconstruct(one(dW), one(dH), None if soft else one(dA), one(dM) if soft else None, one(dX), M, F, T, K, S, 1, pitch, alone)
    assert same_bits(alone[0, :S * M], spec[1, :S * M])
    order = [2, 0, 1]
    moved = torch.full_like(spec, NAN)
    pick = lambda t: t[order].contiguous()
    _array.reconstruct(pick(dW), pick(dH), None if soft else pick(dA), pick(dM) if soft else None, pick(dX), M, F, T, K, S, B, pitch, moved)
    assert same_bits(moved[:, :S * M], spec[order][:, :S * M])


def test_one_target_returns_every_channels_mixture(libs):
    from gcc_nmf_amd import _array
    B, M, F, T, K, S = 1, 3, 33, 10, 8, 1
    X, W, H, am, masks = problem(2, M, F, T, K, S, 5)                 # (file 0 of two: the NaN is in the last file)
    dW, dH, dA, dM, dX = device_operands(X[:1], W[:1], H[:1] + np.float32(0.01), am[:1], masks[:1], 4)
    spec = torch.full((B, 4, dX.shape[2], dX.shape[3], 2), NAN, dtype=torch.float32, device='cuda')
    _array.reconstruct(dW, dH, dA, None, dX, M, F, T, K, S, B, 4, spec)
    assert same_bits(spec[:, :3, :F, :T], dX[:, :, :F, :T]), 'one target: the quotient is exactly 1'


# ---- argument errors: the status code, and nothing written -----------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(libs):
    _, lib = libs
    M, F, T, K, S, B = 3, 33, 5, 4, 2, 2
    Fp, Kp, Tp, Np, P = 48, 64, 64, 64, 3
    X = torch.ones((B, M, Fp, Tp, 2), dtype=torch.float32, device='cuda')
    V = torch.full((B, Fp, Np), NAN, dtype=torch.float32, device='cuda')
    CC = torch.full((B, 2, P * Fp, Tp), NAN, dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(X=X.data_ptr(), M=M, F=F, T=T, batch=B, V=V.data_ptr(), CC=CC.data_ptr())
    feat = lambda **kw: lib.gccnmf_array_features(*[dict(ok, **kw)[k] for k in ('X', 'M', 'F', 'T', 'batch', 'V', 'CC')], st)
    for kw in (dict(M=1), dict(M=9), dict(X=0), dict(V=0, CC=0), dict(F=1), dict(T=0), dict(T=-4), dict(batch=0), dict(batch=-1)):
        assert feat(**kw) == ARG, kw
    assert feat(batch=65536) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(V).all()) and bool(torch.isnan(CC).all())
    W = torch.ones((B, Fp, Kp), dtype=torch.float32, device='cuda')
    H = torch.ones((B, Kp, Np), dtype=torch.float32, device='cuda')
    am = torch.zeros((B, Kp, Tp), dtype=torch.uint8, device='cuda')
    spec = torch.full((B, S * M, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    ok = dict(W=W.data_ptr(), H=H.data_ptr(), argmax=am.data_ptr(), masks=0, X=X.data_ptr(), M=M, F=F, T=T, K=K, S=S, batch=B, pitch=S * M,
              spec=spec.data_ptr())
    order = ('W', 'H', 'argmax', 'masks', 'X', 'M', 'F', 'T', 'K', 'S', 'batch', 'pitch', 'spec')
    rec = lambda **kw: lib.gccnmf_array_reconstruct(*[dict(ok, **kw)[k] for k in order], st)
    for kw in (dict(W=0), dict(H=0), dict(argmax=0), dict(X=0), dict(spec=0), dict(M=1), dict(M=9), dict(F=1), dict(T=0), dict(K=0),
               dict(batch=0), dict(pitch=S * M - 1)):
        assert rec(**kw) == ARG, kw
    for kw in (dict(S=0), dict(S=9, pitch=27), dict(batch=21846)):
        assert rec(**kw) == UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(spec).all())
    assert rec() == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(spec).any())
