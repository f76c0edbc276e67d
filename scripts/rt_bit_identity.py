"""Two builds of the library on every call of tests/rt_checks.CELLS and INFERENCE_CELLS (the real-time block call's stage-test cells):
every buffer a call can write, compared bit for bit.  Each library runs in a process of its own (GCCNMF_HIP_LIB); the parent process
never opens the device.  Used to show that a change leaves the real-time path's bits alone.

    python scripts/rt_bit_identity.py --lib-a /path/to/parent/libgccnmf_hip.so --lib-b gcc_nmf_amd/libgccnmf_hip.so
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

POINTERS = ('block_in', 'block_out', 'in_ring', 'out_ring', 'X', 'Y', 'C', 'HMask', 'argmax', 'tfMask', 'hist', 'hist_pos', 'target', 'gccphat',
            'W', 'cosT', 'sinT', 'window', 'swindow', 'twiddle', 'colsumW', 'Hcoef', 'Rv')


def cells():
    import rt_checks as R
    return list(R.CELLS) + list(R.INFERENCE_CELLS) + [c.with_updates(c.nH + 1) for c in R.INFERENCE_CELLS]


def child(out):
    import torch
    import rt_checks as R
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    res = {}
    for i, c in enumerate(cells()):
        I = R.make_inputs(c)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in I.items()}
        for k, shape in R.output_shapes(c).items():
            d[k] = torch.full(shape, R.SENTINEL_I, dtype=torch.int32, device='cuda') if k == 'argmax' else torch.full(shape, float('nan'), device='cuda')
        rc = lib.gccnmf_rt_process_block_ll(*[d[k].data_ptr() for k in POINTERS], c.N, c.hop, c.B, c.K, c.Kp, c.D, c.Dp, c.Lh, c.mode, c.sep, c.loc,
                                            c.L, c.bits(), c.nH, c.od, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (c.name, rc)
        torch.cuda.synchronize()
        for k in POINTERS:
            res['%03d|%s nH=%d|%s' % (i, c.name, c.nH, k)] = d[k].cpu().numpy()
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib-a')
    ap.add_argument('--lib-b')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    with tempfile.TemporaryDirectory() as tmp:
        got = []
        for tag, path in (('a', a.lib_a), ('b', a.lib_b)):
            out = os.path.join(tmp, tag + '.npz')
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child', out], env=dict(os.environ, GCCNMF_HIP_LIB=os.path.abspath(path)),
                           check=True, timeout=600)
            got.append(np.load(out))
        A, B = got
        assert sorted(A.files) == sorted(B.files)
        differ = [k for k in A.files if A[k].tobytes() != B[k].tobytes()]
        calls = len(set(k.split('|')[0] for k in A.files))
        print(json.dumps(dict(calls=calls, buffers=len(A.files), bytes=int(sum(A[k].nbytes for k in A.files)), buffers_that_differ=len(differ),
                              first=differ[:5])))
        sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
