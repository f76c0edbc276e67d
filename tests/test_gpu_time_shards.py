"""-m gpu: the frame-sharded separation (mode 3: HipTimeShard, separate_time_sharded, shard_frames, time_shard_initial_factors,
stitch_time_shards of gcc_nmf_amd/distributed.py) against the unsplit run, BIT FOR BIT, at every seam and split.

The claim under test is the comment above shard_frames: "the stitched waveform is bit-identical to the single-rank one wherever the
factors are".  Behind the NMF every stage is frame-local -- the STFT of a frame reads that frame's samples, the coherence, the angular
spectrogram's columns, the scores, the arg-max, the reconstruction and the inverse transform work column by column, each output element
a reduction (over bins or atoms) whose order does not know T -- and the overlap-add adds frames in ascending order.  So with the SAME W
and H a sharded run has to reproduce the unsplit run in every bit of every stage; a test of bits needs no derived bar, and a halo frame
added in the wrong order, a frame of H from the wrong channel half or one misplaced sample all show.  The one exception is the time mean
of the angular spectrum, a float64 sum over T whose order does change with the split: it has the bar of gcc_checks.check_mean, and the
picked indexes must be equal.

Launch forms.  The one-shot GEMMs of csrc/gcc.hip (angular spectrogram, scores, reconstruction) choose their kernel by launch size:
gcc_small_launch takes the 128 x 64 ring kernel when batch * ceil(M / 512) * ceil(N / 64) < 256 (and Kd <= 4096), else a 512 x 64
throughput tile.  N is the column count, which does change with the split -- but here batch = 1, M <= 513 (one or two row tiles) and
the widest N is the reconstruction's 2 * S * Tp = 6 * 256 columns of the unsplit 512 / 64 case: 2 * 24 = 48 tiles at most, against the
threshold of 256.  Both sides therefore take the ring kernel in every case and no stage is pinned with tuning key 2; a stage whose bits
differed would be reported by name, not loosened.  The forward and inverse transforms are the radix-2 kernels (n_fft a power of two),
one frame per row, and never see T.

The geometries are tests/time_shard_cases.py (checked on the host by tests/test_distributed_cpu.py, where the float64 oracle finds
the three peaks each case records)."""
import os
import socket

import numpy as np
import pytest

import gcc_checks
import time_shard_cases as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

STAGES = ('X', 'V left', 'V right', 'C', 'angular', 'scores', 'argmax', 'spec', 'frames')     # pipeline order; frame axis last


def _bits(a):
    """The array's bits as integers of the element width (complex: its float parts), so that NaN == NaN and -0 != +0."""
    a = np.ascontiguousarray(a)
    if np.iscomplexobj(a):
        a = a.view(np.float32 if a.dtype == np.complex64 else np.float64)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _frame_stages(shard):
    """Every frame-local stage of a shard that has run masks_and_spectrograms(), on the host, frame axis LAST (complex arrays keep
    their dtype: slice first, then _bits)."""
    e, Tr = shard.e, shard.e.g.T
    V = e.get_V()[0]
    assert V.shape[1] == 2 * Tr
    out = {'X': e.get_X()[0], 'V left': V[:, :Tr], 'V right': V[:, Tr:], 'C': e.get_C()[0], 'angular': e.get_angular()[0][0],
           'scores': e.get_scores()[0], 'argmax': e.get_argmax()[0], 'spec': e.get_spec()[0],
           'frames': np.moveaxis(e.frames[0].cpu().numpy(), 1, -1)}
    assert all(v.shape[-1] == Tr for v in out.values())
    return out


def _load_factors(shard, T, W, H):
    """The given W (F, K) into e.W[0] and the shard's columns of the given H (K, 2T) into e.H[0]: left frames [t0, t1) to columns
    [0, Tr), right frames [T + t0, T + t1) to [Tr, 2 Tr), padding exactly zero."""
    from gcc_nmf_amd.engine import padded
    e, g, t0, t1 = shard.e, shard.e.g, shard.t0, shard.t1
    assert W.shape == (g.F, g.K) and H.shape == (g.K, 2 * T) and g.T == t1 - t0
    Hl = np.concatenate([H[:, t0:t1], H[:, T + t0:T + t1]], axis=1)
    with torch.cuda.device(shard.device):
        e.W[0].copy_(padded(np.asarray(W, np.float32), (g.Fp, g.Kp), shard.device))
        e.H[0].copy_(padded(np.asarray(Hl, np.float32), (g.Kp, g.Np), shard.device))


def replay(x, world, W, H, keep_stages=False, **geometry):
    """The frame-sharded separation of x over `world` shards in ONE process with GIVEN factors, no process group and no NMF: what
    separate_time_sharded does behind train_shared_dictionary, the two collectives done by hand (the shards' angular sums added in
    rank order in float64; every rank handed its predecessor's tail frames).
    -> dict(y, segments [(copy of the segment, start)], idx [per shard], total (D,) float64, T, ranges, stages [per shard] or None)."""
    from gcc_nmf_amd.distributed import HipTimeShard, stitch_time_shards
    shards, sums = [], []
    for rank in range(world):
        s = HipTimeShard(x, rank, world, **geometry)
        s.stft()
        _load_factors(s, s.T_total, W, H)
        sums.append(s.angular_sum().cpu().clone())
        shards.append(s)
    T = shards[0].T_total
    total = sums[0].clone()
    assert total.dtype == torch.float64
    for v in sums[1:]:
        total += v
    segments, idx, stages, tail = [], [], [], None
    for s in shards:
        s.set_angular_mean(total / float(T))
        s.masks_and_spectrograms()
        mine = s.tail_frames()
        seg, start = s.overlap_add(tail)
        segments.append((np.array(seg), int(start)))              # a view of a pinned buffer that the next call reuses: copy
        tail = mine
        idx.append([int(i) for i in s.tdoa_indexes()])
        stages.append(_frame_stages(s) if keep_stages else None)
    y = stitch_time_shards(segments, shards[0].S, T, shards[0].hop)
    return dict(y=y, segments=segments, idx=idx, total=total.numpy(), T=T, ranges=[(s.t0, s.t1) for s in shards], stages=stages)


def _first_difference(got, want):
    bad = np.argwhere(_bits(got) != _bits(want))
    return None if not len(bad) else tuple(int(i) for i in bad[0])


@pytest.mark.parametrize('name', list(C.CASES))
def test_shards_with_given_factors_are_the_unsplit_run_bit_for_bit(name):
    """R shards with the unsplit run's own W and H against the unsplit run: every frame-local stage of every shard, then every sample
    of the stitched waveform, in bits (module docstring: both sides on the ring kernel, nothing pinned).  The NMF runs once, on the
    one-shard side (separate_time_sharded, 6 iterations); its factors, read back, are the given ones."""
    from gcc_nmf_amd.distributed import HipTimeShard, separate_time_sharded, stitch_time_shards
    n_fft, hop, world, n, numTDOAs = C.CASES[name]
    T, halo, split = C.EXPECTED[name]
    geometry = dict(windowSize=n_fft, hopSize=hop, numTDOAs=numTDOAs, numTargets=C.NUM_TARGETS, dictionarySize=C.DICTIONARY_SIZE)
    x = C.mixture(n)
    S = C.NUM_TARGETS
    print('%s: T = %d, halo = %d, split = %s, %d samples' % (name, T, halo, '/'.join(map(str, split)), n))

    one = HipTimeShard(x, 0, 1, **geometry)
    assert (one.T_total, one.halo, one.t1 - one.t0) == (T, halo, T)
    seg1, start1 = separate_time_sharded(one, 6)
    y1 = stitch_time_shards([(np.array(seg1), start1)], S, T, hop)
    W, H = [a[0] for a in one.e.get_WH()]
    ref = _frame_stages(one)
    V1 = one.e.get_V()[0]
    ang1, mean1 = [a[0] for a in one.e.get_angular()]
    idx1 = [int(i) for i in one.tdoa_indexes()]
    # nothing vacuous
    assert np.isfinite(y1).all() and np.isfinite(W).all() and np.isfinite(H).all(), 'the unsplit run is not finite'
    assert idx1 == C.PEAKS[name], 'the unsplit run picked %s, the float64 oracle %s' % (idx1, C.PEAKS[name])
    assert start1 == -(n_fft // 2), '%s: the unsplit segment starts at %d, not at the centre trim -%d' % (name, start1, n_fft // 2)
    assert seg1.shape == (S, 2, (T - 1) * hop + n_fft) and y1.shape == (S, 2, hop * (T - 1)), (seg1.shape, y1.shape)

    r = replay(x, world, W, H, keep_stages=True, **geometry)
    assert r['T'] == T and [b - a for a, b in r['ranges']] == split, (r['T'], r['ranges'])

    # stage by stage, shard by shard: the first stage (pipeline order) that differs is named
    for stage in STAGES:
        for rank, ((t0, t1), got) in enumerate(zip(r['ranges'], r['stages'])):
            if stage == 'V right':                                     # stated on the unsplit V's own columns: T + t0 .. T + t1
                want = V1[:, T + t0:T + t1]
            else:
                want = ref[stage][..., t0:t1]
            assert got[stage].shape == want.shape and got[stage].dtype == want.dtype, (stage, rank, got[stage].shape, want.shape)
            where = _first_difference(got[stage], want)
            assert where is None, ('%s: stage %r is the first that differs, on rank %d (frames [%d, %d) of %d): first at %s of %s'
                                   % (name, stage, rank, t0, t1, T, where, _bits(want).shape))

    # the time mean: the rank-ordered float64 sum against T x the unsplit mean, and against the float64 mean of the (identical) rows
    bound = 4.0 * (T + 1) * gcc_checks.U64 * np.mean(np.abs(ang1.astype(np.float64)), axis=-1)
    err = np.abs(r['total'] - T * mean1)
    assert (err <= T * bound).all(), '%s: angular sum off at TDOA %d: %r vs %r' % (name, int(np.argmax(err > T * bound)),
                                                                                  r['total'][np.argmax(err > T * bound)],
                                                                                  T * mean1[np.argmax(err > T * bound)])
    gcc_checks.check_mean(r['total'] / T, ang1, what='%s: sum of the shards / T' % name)
    assert all(i == idx1 for i in r['idx']), '%s: the shards picked %s, the unsplit run %s' % (name, r['idx'], idx1)

    # samples: the segments tile [-(n_fft // 2), ...), the last one runs to the end of its last frame, every sample equal in bits
    starts, lens = [s for _, s in r['segments']], [seg.shape[2] for seg, _ in r['segments']]
    assert starts[0] == -(n_fft // 2), '%s: the first segment starts at %d, not at the centre trim -%d' % (name, starts[0], n_fft // 2)
    for k in range(world - 1):
        assert starts[k] + lens[k] == starts[k + 1], '%s: segments %d and %d leave a gap or overlap: %s + %s' % (name, k, k + 1, starts, lens)
        assert lens[k] == split[k] * hop, '%s: segment %d is %d long, not its %d frames x hop' % (name, k, lens[k], split[k])
    assert lens[-1] == (split[-1] - 1) * hop + n_fft, '%s: the last segment is %d long' % (name, lens[-1])
    assert r['y'].shape == y1.shape
    where = _first_difference(r['y'], y1)
    if where is not None:
        seam = max([s for s in starts if s <= where[2]])
        raise AssertionError('%s: every stage equal, but the stitched waveform differs first at %s (segment starting at %d, %d samples '
                             'behind its seam; n_fft - hop = %d): %r vs %r' % (name, where, seam, where[2] - seam, n_fft - hop,
                                                                               r['y'][where], y1[where]))
    for s in starts[1:]:
        assert np.any(y1[:, :, s:s + n_fft - hop] != 0), '%s: the %d samples behind the seam at %d are all zero' % (name, n_fft - hop, s)
    print('%s: %d stages x %d shards and %d x 2 x %d samples equal in bits; sum of the shards within %.2f of the mean bar'
          % (name, len(STAGES), world, S, y1.shape[2], float(np.max(err / (T * bound)))))


def test_constructor_refuses_a_shard_shorter_than_its_halo():
    """A shard of fewer than max(halo, 2) frames raises the documented ValueError on every rank that is that short; one frame more
    builds.  1024 / 300 (halo 3) and 1024 / 512 (halo 1: the 2 is what binds)."""
    from gcc_nmf_amd.distributed import HipTimeShard
    for n_fft, hop, need in ((1024, 300, 3), (1024, 512, 2)):
        world = 3
        short = np.zeros((2, n_fft + hop * (world * (need - 1) - 1)), np.float32)            # T = world * (need - 1)
        for rank in range(world):
            with pytest.raises(ValueError, match='shorter than the overlap-add halo'):
                HipTimeShard(short, rank, world, windowSize=n_fft, hopSize=hop, dictionarySize=64)
        enough = np.zeros((2, n_fft + hop * (world * need - 1)), np.float32)                 # T = world * need
        for rank in range(world):
            s = HipTimeShard(enough, rank, world, windowSize=n_fft, hopSize=hop, dictionarySize=64)
            assert s.t1 - s.t0 == need and s.halo == -(-n_fft // hop) - 1
        # uneven: T = world * need - 1 leaves the LAST rank one frame short, and only that rank refuses
        uneven = np.zeros((2, n_fft + hop * (world * need - 2)), np.float32)
        HipTimeShard(uneven, 0, world, windowSize=n_fft, hopSize=hop, dictionarySize=64)
        with pytest.raises(ValueError, match='shorter than the overlap-add halo'):
            HipTimeShard(uneven, world - 1, world, windowSize=n_fft, hopSize=hop, dictionarySize=64)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_three_ranks_over_gloo_are_the_replay_of_their_own_factors(tmp_path):
    """separate_time_sharded itself through the real collectives: three PROCESSES on GPU 0 over gloo, 1024 / 300 (a middle rank, a hop
    that does not divide n_fft), K = 64, 5 iterations.  W is the same in bits on every rank (every rank applies the same update to the
    same all-reduced [num || den]), so are the TDOA indexes, and one shard replaying the gathered factors reproduces the three-rank
    stitched waveform in every bit -- the all-reduce of the angular sum, the all-gather and tails[rank - 1] with no bar for the
    iterated factors (whose own arithmetic tests/test_gpu_shared_protocol.py checks element by element)."""
    import subprocess
    import sys
    from conftest import REPO
    from gcc_nmf_amd.distributed import stitch_time_shards
    n_fft, hop, world, n, K, iters, S = 1024, 300, 3, 24000, C.DICTIONARY_SIZE, 5, C.NUM_TARGETS
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(REPO, 'tests', 'time_shard_worker.py'), str(tmp_path)] + [
               str(v) for v in (n, K, iters, n_fft, hop, S, 1)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    parts = [np.load(tmp_path / ('time_rank%d.npz' % k)) for k in range(world)]
    T = int(parts[0]['T'])
    ranges = [(int(q['t0']), int(q['t1'])) for q in parts]
    assert T == 77 and [b - a for a, b in ranges] == [26, 26, 25] and ranges[0][0] == 0 and ranges[-1][1] == T
    for k in range(1, world):
        assert _first_difference(parts[k]['W'], parts[0]['W']) is None, 'W of rank %d differs from rank 0 at %s' % (
            k, _first_difference(parts[k]['W'], parts[0]['W']))
        assert parts[k]['idx'].tolist() == parts[0]['idx'].tolist(), 'rank %d picked %s, rank 0 %s' % (k, parts[k]['idx'], parts[0]['idx'])
    assert parts[0]['idx'].tolist() == C.PEAKS['1024/300 x3']
    H = np.full((K, 2 * T), np.nan, np.float32)
    for q, (t0, t1) in zip(parts, ranges):
        assert q['H'].shape == (K, 2 * (t1 - t0))
        H[:, t0:t1], H[:, T + t0:T + t1] = q['H'][:, :t1 - t0], q['H'][:, t1 - t0:]
    assert np.isfinite(H).all() and np.isfinite(parts[0]['W']).all()
    segments = [(q['seg'], int(q['start'])) for q in parts]
    for k in range(world - 1):
        assert segments[k][1] + segments[k][0].shape[2] == segments[k + 1][1], 'segments %d and %d do not tile' % (k, k + 1)
    y3 = stitch_time_shards(segments, S, T, hop)
    r = replay(C.mixture(n), 1, parts[0]['W'], H, windowSize=n_fft, hopSize=hop, numTargets=S, dictionarySize=K)
    assert r['idx'][0] == parts[0]['idx'].tolist(), 'the replay picked %s, the ranks %s' % (r['idx'][0], parts[0]['idx'].tolist())
    assert np.isfinite(y3).all() and r['y'].shape == y3.shape
    where = _first_difference(y3, r['y'])
    if where is not None:
        starts = [s for _, s in segments]
        seam = max([s for s in starts if s <= where[2]])
        raise AssertionError('three ranks over gloo differ from the replay of their own factors first at %s (segment starting at %d, %d '
                             'samples behind its seam; n_fft - hop = %d): %r vs %r' % (where, seam, where[2] - seam, n_fft - hop,
                                                                                       y3[where], r['y'][where]))
    for _, s in segments[1:]:
        assert np.any(y3[:, :, s:s + n_fft - hop] != 0)
