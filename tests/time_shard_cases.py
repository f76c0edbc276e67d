"""The frame-sharded (mode 3) geometries that tests/test_gpu_time_shards.py replays on the device and tests/test_distributed_cpu.py
checks on the host: plain data and arithmetic, no torch and no device.

Each case: (n_fft, hop, world, numSamples, numTDOAs).  numSamples is chosen so that T = 1 + (numSamples - n_fft) // hop and the balanced
split have the property the case is there for; ``describe`` restates T, the halo and the split from the numbers alone, and the tests
compare them with what the package computes."""

NUM_TARGETS = 3               # synthetic_mixture's three delays (-20, 3, 27 samples): three peaks of the mean angular spectrum
DICTIONARY_SIZE = 64
MIXTURE_INDEX = 11

CASES = {
    # a middle rank and an uneven split: T = 91 -> 31 / 30 / 30
    '1024/256 x3': (1024, 256, 3, 24100, 128),
    # three shards of exactly `halo` frames, whose tail is all of their frames: T = 29 -> 8 / 7 / 7 / 7
    '1024/128 x4': (1024, 128, 4, 4700, 128),
    # the hop does not divide n_fft (halo = ceil(1024 / 300) - 1 = 3); a seam at t0 * 300 is no multiple of n_fft / 4: T = 77 -> 26 / 26 / 25
    '1024/300 x3': (1024, 300, 3, 24000, 128),
    # halo 1, shards of 3 and 2 = max(halo, 2) frames: T = 17 -> 3 / 3 / 3 / 2 / 2 / 2 / 2
    '1024/512 x7': (1024, 512, 7, 9300, 64),
    # off the 1024 path, a long halo: T = 243 -> 49 / 49 / 49 / 48 / 48
    '512/64 x5': (512, 64, 5, 16000, 128),
    # a small window and a hop that does not divide it (halo = ceil(2.56) - 1 = 2): T = 159 -> 80 / 79
    '256/100 x2': (256, 100, 2, 16100, 64),
    # the eight-rank split, T no multiple of 8: T = 122 -> 16 / 16 / 15 x 6
    '1024/256 x8': (1024, 256, 8, 32000, 128),
}

# what each case is there for, restated from the numbers: (T, halo, split)
EXPECTED = {
    '1024/256 x3': (91, 3, [31, 30, 30]),
    '1024/128 x4': (29, 7, [8, 7, 7, 7]),
    '1024/300 x3': (77, 3, [26, 26, 25]),
    '1024/512 x7': (17, 1, [3, 3, 3, 2, 2, 2, 2]),
    '512/64 x5': (243, 7, [49, 49, 49, 48, 48]),
    '256/100 x2': (159, 2, [80, 79]),
    '1024/256 x8': (122, 3, [16, 16, 15, 15, 15, 15, 15, 15]),
}

# the three peaks of the mean angular spectrum that the float64 oracle picks (tests/test_distributed_cpu.py recomputes them); the
# unsplit device run must find the same, so no case compares two runs that found nothing
PEAKS = {
    '1024/256 x3': [27, 59, 91],
    '1024/128 x4': [27, 59, 90],
    '1024/300 x3': [27, 59, 91],
    '1024/512 x7': [13, 29, 45],
    '512/64 x5': [27, 59, 91],
    '256/100 x2': [13, 29, 45],
    '1024/256 x8': [27, 59, 91],
}


def describe(name):
    """(T, halo, split) of a case by integer arithmetic alone."""
    n_fft, hop, world, n, _ = CASES[name]
    T = 1 + (n - n_fft) // hop
    halo = (n_fft + hop - 1) // hop - 1
    q, r = divmod(T, world)
    return T, halo, [q + (1 if k < r else 0) for k in range(world)]


def mixture(n):
    from gcc_nmf_amd.synthetic import synthetic_mixture
    return synthetic_mixture(MIXTURE_INDEX, numSamples=n)
