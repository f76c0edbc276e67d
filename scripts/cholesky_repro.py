"""Why evaluation._solve is a batched LU and not Cholesky -> profiles/r22a_cholesky_repro.json.

Two 144 x 144 float64 Gram matrices of delayed white-plus-filtered signals (3 sources x 2 channels x 24 taps, the shape at which the
scoring tests first showed SIR and SAR moving between two calls on the same waveforms), uploaded once.  Per repeat, on the SAME device
tensors: torch.linalg.cholesky_ex + cholesky_solve and torch.linalg.solve -- the info words, the residual max|G x - d|, and whether the
factor / the solution has the bits of the first repeat.  Between repeats a freed allocation is filled with NaN, so that a routine
that reads workspace it has not written shows it.  The float64 host solve (numpy) gives the residual to expect.

    python scripts/cholesky_repro.py [--repeats 6] [--out profiles/r22a_cholesky_repro.json]

Needs a ROCm device."""
import argparse
import json
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gram(seed, J=3, C=2, L=24, n=4000):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(J):
        src = rng.standard_normal(n + 3)
        for _ in range(C):
            x = np.convolve(src, rng.standard_normal(4) * [1.0, 0.5, 0.25, 0.125])[3:3 + n] + 0.3 * rng.standard_normal(n)
            for tau in range(L):
                rows.append(np.concatenate([np.zeros(tau), x, np.zeros(L - 1 - tau)]))
    D = np.stack(rows)
    return D @ D.T, D @ rng.standard_normal((n + L - 1, J * C))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r22a_cholesky_repro.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a ROCm device'
    pairs = [gram(0), gram(1)]
    G_h, d_h = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    x_h = np.linalg.solve(G_h, d_h)
    rec = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shape=list(G_h.shape),
               cond=[float(np.linalg.cond(g)) for g in G_h], host_residual=float(np.abs(G_h @ x_h - d_h).max()), repeats=[])
    dev = torch.device('cuda:0')
    G, d = torch.from_numpy(G_h).to(dev), torch.from_numpy(d_h).to(dev)
    first = {}

    def same(name, t):
        v = t.cpu().numpy()
        return bool(np.array_equal(v, first.setdefault(name, v), equal_nan=True))

    for rep in range(a.repeats):
        if rep:
            junk = torch.full((rep * 1000003 + 17,), float('nan'), dtype=torch.float64, device=dev)
            del junk
        Lc, info = torch.linalg.cholesky_ex(G)
        x = torch.cholesky_solve(d, Lc)
        y = torch.linalg.solve(G, d)
        torch.cuda.synchronize()
        rec['repeats'].append(dict(
            cholesky_info=info.tolist(), cholesky_residual=float(torch.nan_to_num(G @ x - d, nan=float('inf')).abs().max()),
            cholesky_factor_same_bits_as_first=same('L', Lc), cholesky_solution_same_bits_as_first=same('x', x),
            cholesky_against_host=float(np.nan_to_num(np.abs(x.cpu().numpy() - x_h), nan=np.inf).max()),
            lu_residual=float((G @ y - d).abs().max()), lu_same_bits_as_first=same('y', y),
            lu_against_host=float(np.abs(y.cpu().numpy() - x_h).max()), input_same_bits_as_first=same('G', G)))
    bad = [r for r in rec['repeats'] if any(r['cholesky_info']) or r['cholesky_residual'] > 1e3 * rec['host_residual']]
    rec['cholesky_wrong_repeats'], rec['lu_wrong_repeats'] = len(bad), len([r for r in rec['repeats'] if r['lu_residual'] > 1e3 * rec['host_residual']])
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(rec, sort_keys=True))


if __name__ == '__main__':
    main()
