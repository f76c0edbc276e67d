"""The case table of tests/test_gpu_chained_small_shapes.py: every chained form of gccnmf_klnmf and gccnmf_klnmf_ragged (include/gccnmf_hip.h, tuning
keys 21 / 23 / 24) at the SMALLEST shapes that reach it -- a few hundred kilobytes per call -- where the hand-over logic has the least slack: one
column tile per file, one file per XCD list, lists of unequal length, a last column tile of 1 / 32 / 33 columns, N an exact multiple of 64, two row
tiles of K2, F = 257 / 385, all eight instantiations of the short-dictionary chain, ragged batches whose files decide `narrow` each for itself.
No torch and no device here: tests/test_chained_small_cases_host.py checks this table against gccnmf_klnmf_plan, which is host code.

THE PROBLEMS come from klnmf_stages_restatement.problem: a distinct W0, H0 and V per file, never a silent frame.
  * A call of ONE iteration keeps problem()'s silent bin (one all-zero row of V per file): that row of W must come out exactly 0.
  * A call of MORE iterations cannot keep it.  The first W update makes the bin's row of W exactly 0, so the second iteration forms V / (W.H) =
    0 / 0 in the whole bin, the NaN enters K2's sum over the bins, and W and H are NaN throughout -- in the float64 reference too
    (tests/test_chained_small_cases_host.py::test_a_silent_bin_does_not_survive_a_second_iteration shows it; DESIGN 2b says the same of the
    shared-dictionary run).  NaN compares unequal to itself, so such a call would pin nothing.  Those calls use lines=False -- the isolated exact
    zeros of V stay -- and positive_rows() lifts any row of V that is zero as a whole (at N = 1 every isolated zero is one)."""
import collections

import numpy as np

import klnmf_stages_restatement as S

DEFAULTS = {2: 0, 3: 1, 9: 1, 10: 1, 16: 1, 17: 1, 21: 1, 23: 1, 24: 2048}      # every tuning key a case may set (never 22 or 25: the lab hooks)
EPS = 1e-16
DIRECT, K1K2, K3K4A, CHAINED = 1, 2, 4, 8                                         # bits of gccnmf_klnmf_plan

# one call: the tuning keys beside the case's own, the plan bits (of the low four) it must show, and whether it is compared with the plain call
Call = collections.namedtuple('Call', 'name keys plan compared')


def n_class(N):
    """what a file's column count means to the 64-column tiles: (column tiles, columns of the last one as 1 | narrow <= 32 | 33-63 | full)"""
    last = N - (-(-N // 64) - 1) * 64
    return -(-N // 64), '1' if last == 1 else 'narrow' if last <= 32 else 'full' if last == 64 else 'wide'


def positive_rows(V):
    """a writable copy of V (files, F, N) in which no row is zero as a whole: a zero row of V is lifted to 0.25 (see the module docstring)"""
    V = np.array(V)
    V[~V.any(axis=2)] = 0.25
    return V


def problem(F, N, K, files, iterations):
    """V, W0, H0 (float32, per file) of a call of `iterations` iterations: with problem()'s silent bin for ONE iteration, without it for more"""
    V, W, H, _ = S.problem(F, N, K, files, lines=iterations == 1, frames=False)
    return (np.array(V) if iterations == 1 else positive_rows(V)), np.array(W), np.array(H)


# ---- B: the throughput chain (K >= 256 a multiple of 128), bit for bit the plain call under key 2 = 1 ---------------------------------------------
#   (257, 256)  K2 on half-height tiles, Fm = 256         (385, 384)  K2 on one full-height row tile, Fm = 384
#   (513, 640)  two row tiles of K2, five atom tiles of K4   (513, 256)  the workload's F with the smallest chain-capable dictionary
#   N: one column tile of 1 / 32 / 33 / 64 columns, two with a last one of 1 / 32 / 33, three with a last one of 2
#   B: 8 one file per list | 9, 13 lists of unequal length, spread by rule | 16, 24 whole-file lists by rule (chain_list_mode)
THROUGHPUT_FK = [(257, 256), (385, 384), (513, 640), (513, 256)]
THROUGHPUT_N = [1, 32, 33, 64, 65, 96, 97, 130]
THROUGHPUT_B = [8, 9, 13, 16, 24]
THROUGHPUT_KEYS = {2: 1}
PLAIN = Call('plain', {21: 0}, 0, False)
CHAIN_PAIRS = [(2, 1), (4, 1), (8, 1), (8, 2), (8, 3), (8, 0)]                    # (key 21, key 23)

ThroughputCase = collections.namedtuple('ThroughputCase', 'F N K B iterations alpha calls oracle')


def throughput_cases():
    """Case (i, j) = THROUGHPUT_FK[i] x THROUGHPUT_N[j]; with s = i + j: the batch is THROUGHPUT_B[s mod 5] and the call has 5 iterations for even
    s, 1 for odd s -- every N and every batch with every (F, K), either iteration count with every batch.  Every case runs the plain call, the
    whole call chained (key 21 = 8) twice, and key 23 = 0 (the plain launch's lists: a chained form for a batch that is a multiple of 8, else the
    plan bit must be clear and the call is the plain one); s mod 4 picks the rest, so that the four (F, K) of one N run every pair between them:
        0: key 21 = 2, key 23 = 2, key 24 = 1      1: key 21 = 4, key 23 = 2      2: key 21 = 4, key 23 = 3, key 24 = 3      3: key 21 = 2, key 23 = 3
    (key 24, iterations per launch, is only laid over the 5-iteration calls: 0 and 2).  N = 65 runs with sparsity_alpha = 0.2, the others with 0.
    One 5-iteration case per (F, K) -- N = 130, or 97 where 130 has one iteration -- gives its first and its last file the oracle's own initial
    factors (`oracle`), so that the plain call, the reference side of every comparison here, is itself compared with performKLNMF."""
    cases = []
    for i, (F, K) in enumerate(THROUGHPUT_FK):
        for j, N in enumerate(THROUGHPUT_N):
            s = i + j
            B, iterations = THROUGHPUT_B[s % 5], (5, 1)[s % 2]
            whole = {21: 8}
            calls = [PLAIN, Call('whole call', whole, CHAINED, True), Call('whole call again', whole, CHAINED, True),
                     Call('plain lists', {21: 8, 23: 0}, CHAINED if B % 8 == 0 else 0, B % 8 == 0)]
            k21, k23 = ((2, 2), (4, 2), (4, 3), (2, 3))[s % 4]
            calls.append(Call('K1 | K2' if k21 == 2 else 'one iteration', {21: k21}, CHAINED, True))
            calls.append(Call('spread lists' if k23 == 2 else 'whole-file lists', {21: 8, 23: k23}, CHAINED, True))
            if s % 4 in (0, 2):
                calls.append(Call('%d per launch' % (1 + s % 4), {21: 8, 24: 1 + s % 4}, CHAINED, True))
            oracle = iterations == 5 and N == (130 if (i + 7) % 2 == 0 else 97)
            cases.append(ThroughputCase(F, N, K, B, iterations, 0.2 if N == 65 else 0.0, tuple(calls), oracle))
    return cases


def oracle_factors(F, N, K, seed):
    """oracle.gccnmf_oracle.initKLNMF restated (gcc_nmf_amd.engine.klnmf_initial_factors is the same): what performKLNMF(..., seedValue=seed) starts from"""
    rs = np.random.RandomState(seed)
    W = rs.random_sample((F, K)).astype(np.float32) + EPS
    H = rs.random_sample((K, N)).astype(np.float32) + EPS
    return W.astype(np.float32), H.astype(np.float32)


def throughput_problem(case):
    V, W, H = problem(case.F, case.N, case.K, case.B, case.iterations)
    if case.oracle:
        for b in (0, case.B - 1):
            W[b], H[b] = oracle_factors(case.F, case.N, case.K, b)
    return V, W, H


# ---- C: the short-dictionary chain (K <= 128), bit for bit the plain call at ANY batch under keys 16 = 17 = 2 ---------------------------------------
# gccnmf_short_chain_kernel<KB, atoms per W-update group>: KB = ceil(K / 32); 32 atoms per group from batch * Kp / 32 >= 256 on, else 16 (plan_klnmf's
# short_group, the rule of launch_update_w).  The chain exists for 8 <= batch and batch * Kp / 64 < 256.
SHORT_KEYS = {16: 2, 17: 2}
SHORT_SHAPES = [((129, 65, 20), (8, 130)), ((257, 64, 33), (13, 128)), ((385, 130, 96), (24, 64)), ((385, 1, 65), (9,)),
                ((513, 130, 128), (9, 70)), ((513, 1, 100), (8,))]
SHORT_REFUSED = (129, 65, 33, 16)      # Fm / 64 = 2 slabs hold 32 atoms' worth of U columns, 64 are needed: no slab launch, so no chain either

ShortCase = collections.namedtuple('ShortCase', 'F N K B iterations alpha calls KB group')


def short_group(K, B):
    Kp = -(-K // 64) * 64
    return 32 if B * (Kp // 32) >= 256 else 16


def short_cases():
    """Every (shape, batch) above at 1 and at 4 iterations: the plain call (key 21 = 0), the chain (key 21 = 8) twice and, at 4 iterations, the
    chain at one iteration per launch (key 24 = 1).  sparsity_alpha = 0.2 at (385, 130, 96) x 24, else 0.  The refused shape runs the same calls:
    the slab-launch bit and the chain bit stay clear, the call is the plain one and must still succeed and agree."""
    cases = []
    for (F, N, K), batches in SHORT_SHAPES + [(SHORT_REFUSED[:3], SHORT_REFUSED[3:])]:
        chained = (F, N, K) != SHORT_REFUSED[:3]
        plain, chain = (K1K2 | K3K4A, K1K2 | K3K4A | CHAINED) if chained else (K1K2, K1K2)
        for B in batches:
            for iterations in (1, 4):
                calls = [Call('plain', {21: 0}, plain, False), Call('chain', {21: 8}, chain, True), Call('chain again', {21: 8}, chain, True)]
                if iterations > 1:
                    calls.append(Call('1 per launch', {21: 8, 24: 1}, chain, True))
                cases.append(ShortCase(F, N, K, B, iterations, 0.2 if (F, B) == (385, 24) else 0.0, tuple(calls), -(-K // 32),
                                       short_group(K, B) if chained else 0))
    return cases


# ---- D: the ragged batch, every file bit for bit what the plain call gives it in a uniform batch of the files of its length ---------------------------
RAGGED_FK = [(257, 256), (513, 384)]
RAGGED_NMAX, RAGGED_ITERATIONS = 130, 4
RAGGED_KEYS = {2: 1, 10: 0}            # (key 10 = 0: a reference batch of one or two files stays on the throughput tile, off the direct kernels)
RAGGED_LENGTHS = [
    [1, 32, 33, 64, 65, 96, 97, 130, 130, 97, 96, 65, 64, 33, 32, 1],      # every length class twice: two files per XCD list
    [130, 1, 64, 33, 96, 65, 32, 97, 130],                                  # one file per list plus one
]


def ragged_lists(lengths):
    """gccnmf_klnmf_ragged's dealing restated (csrc/nmf.hip): longest first (ties: the lower file), each file to the list with the fewest column
    tiles so far (ties: the lower list); a list serves its files in ascending order."""
    lists, load = [[] for _ in range(8)], [0] * 8
    for f in sorted(range(len(lengths)), key=lambda f: -lengths[f]):
        best = min(range(8), key=lambda l: (load[l], l))
        lists[best].append(f)
        load[best] += -(-lengths[f] // 64)
    return [sorted(l) for l in lists]


def ragged_problem(F, K, lengths):
    """per file (V (F, n), W0 (F, K), H0 (K, n)): file f is the next file of problem(F, n, K, ...) for its own n = lengths[f] -- files of one length
    are distinct files of ONE uniform problem, which is the reference batch of that length.  -> files, {n: [file indexes in batch order]}"""
    by_length = collections.OrderedDict()
    for f, n in enumerate(lengths):
        by_length.setdefault(n, []).append(f)
    files = [None] * len(lengths)
    for n, idx in by_length.items():
        V, W, H = problem(F, n, K, max(len(idx), 2), RAGGED_ITERATIONS)
        for b, f in enumerate(idx):
            files[f] = (V[b], W[b], H[b])
    return files, by_length
