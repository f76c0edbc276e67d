"""Two builds of libgccnmf_hip.so and libgccnmf_array.so on the calls that share ratio_kernel.h and phat.h: the SHA-256 of every output
buffer, padding included, of gccnmf_reconstruct (ratio mode), gccnmf_array_reconstruct, gccnmf_coherence and gccnmf_array_features, on the
shapes of tests/test_gpu_array_stages.py (CASES in both forms, the stereo call on each case's channel 0; M = 2 ... 8, T = 2 / 64 / 67 at
F = 33 for the features).  Each build runs in a process of its own, the second only after the first has ended well; the parent process
never opens the device.  Used to show that a change leaves these bits alone.

    python scripts/reconstruct_bit_identity.py --lib-a /path/to/parent/gcc_nmf_amd --lib-b gcc_nmf_amd
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def child(lib_dir):
    import torch
    import test_gpu_array_stages as G
    from gcc_nmf_amd import _array, _hip
    _hip.LIB_PATH, _array.LIB_PATH = [os.path.join(lib_dir, n) for n in ('libgccnmf_hip.so', 'libgccnmf_array.so')]
    nan = lambda *shape: torch.full(shape, G.NAN, dtype=torch.float32, device='cuda')

    def emit(case, **buffers):
        torch.cuda.synchronize()
        for name, t in buffers.items():
            print('%s|%s %s' % (case, name, hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()), flush=True)

    B = 3
    for M, F, K, T, S in G.CASES:
        X, W, H, am, masks = G.problem(B, M, F, T, K, S, 1000 * M + 10 * K + S)
        pitch = S * M + 2
        dW, dH, dA, dM, dX = G.device_operands(X, W, H, am, masks, pitch)
        Fp, Tp = dX.shape[2], dX.shape[3]
        Hs = torch.zeros((B, dH.shape[1], G.rup(2 * T, 64)), dtype=torch.float32, device='cuda')       # channel 0 twice: a stereo problem
        Hs[:, :, :T] = Hs[:, :, T:2 * T] = dH[:, :, :T]
        Xs = dX[:, [0, 0]].contiguous()
        for soft in (False, True):
            a, m = (None, dM) if soft else (dA, None)
            array, stereo = nan(B, pitch, Fp, Tp, 2), nan(B, 2 * S, Fp, Tp, 2)
            _array.reconstruct(dW, dH, a, m, dX, M, F, T, K, S, B, pitch, array)
            _hip.reconstruct(dW, Hs, a, m, Xs, None, F, T, K, S, B, stereo, mode='ratio')
            emit('reconstruct M%d F%d K%d T%d S%d %s' % (M, F, K, T, S, 'soft' if soft else 'one-hot'), array=array, stereo=stereo)
    F, Fp = 33, 48
    for M in range(2, 9):
        for T in (2, 64, 67):
            dX = G.dev(G.padded_X(G.feature_spectra(B, M, F, T, 10 * M + T), Fp, G.rup(T, 64)))
            Tp, P = dX.shape[3], M * (M - 1) // 2
            V, CC, stereo = nan(B, Fp, G.rup(M * T, 64)), nan(B, 2, P * Fp, Tp), nan(B, 2, Fp, Tp)
            _array.features(dX, M, F, T, B, V, CC)
            _hip.coherence(dX[:, :2].contiguous(), F, T, B, stereo)
            emit('features M%d T%d' % (M, T), V=V, CC=CC, stereo_CC=stereo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib-a', help='directory with libgccnmf_hip.so and libgccnmf_array.so of one build')
    ap.add_argument('--lib-b', help='... of the other')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    got = []
    for d in (a.lib_a, a.lib_b):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', os.path.abspath(d)], stdout=subprocess.PIPE, text=True,
                             check=True, timeout=600)
        got.append(dict(line.rsplit(' ', 1) for line in run.stdout.splitlines()))
    A, B = got
    for k in A:
        print(k, A[k], 'same' if B.get(k) == A[k] else 'DIFFERS: %s' % B.get(k))
    differ = [k for k in sorted(set(A) | set(B)) if A.get(k) != B.get(k)]
    print(json.dumps(dict(cases=len(set(k.split('|')[0] for k in A)), buffers=len(A), buffers_that_differ=len(differ), first=differ[:5])))
    sys.exit(1 if differ or not A else 0)


if __name__ == '__main__':
    main()
