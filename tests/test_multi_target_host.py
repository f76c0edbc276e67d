"""Multiple mode (TARGET_MODE_MULTIPLE) without a device: the frames_mode rules of gccnmf_rt_process_block_ll (checked before any
HIP call), the Python argument checks, and the ABI that did not grow."""
import ctypes

import numpy as np
import pytest

from gcc_nmf_amd import _hip


def _call(bits, target_mode=1):
    """gccnmf_rt_process_block_ll on host scratch with an otherwise valid single-stream configuration (reference: 1024 / 512 / 512,
    K = 128, D = 64): only the frames_mode word and target_mode decide.  Called only where the answer is GCCNMF_ERR_ARG."""
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return _hip.lib().gccnmf_rt_process_block_ll(*([p] * 23), 1024, 512, 512, 128, 128, 64, 64, 128, target_mode, 1, 1, 6, bits, 0, 2,
                                                 None)


MULTI = 1 << 20


@pytest.mark.parametrize('bits,mode', [
    (MULTI, 0), (MULTI, 2), (MULTI | (2 << 21), 2),          # the multi-target layout needs target_mode 1
    (1 << 21, 1), (7 << 21, 1), (3 << 21, 2),                # target count without the layout
    (MULTI | (1 << 24), 1), (MULTI | (7 << 21) | (1 << 24), 1),   # N > 8 does not fit bits 21..23; nothing above bit 23
    (MULTI | 8 | 1, 1),                                      # bank layout with frames mode stays an error
])
def test_frames_mode_rules(bits, mode):
    assert _call(bits, mode) == 1                            # GCCNMF_ERR_ARG


def test_num_sources_and_target_indexes_are_checked():
    from gcc_nmf_amd import realtime as rt
    for n in (0, 9, 2.5, -1, True):
        with pytest.raises(ValueError):
            rt._check_num_sources(n)
    assert [rt._check_num_sources(n) for n in (1, 8, 3.0)] == [1, 8, 3]
    # the constructor checks numSources before it looks for a device
    W = np.ones((513, 8), np.float32)
    with pytest.raises(ValueError):
        rt.GCCNMFProcessor(16000, 1024, 1, {'P': {8: W}}, 'P', 8, 0, 0.1, True, 6, numSources=9)
    for bad in ([1], [1, 2, 3], [1.5, 2], [-1, 2], [3, 64], [np.nan, 2], 'ab', [[1, 2], [3, 4]], None):
        with pytest.raises(ValueError):
            rt._check_target_indexes(bad, 2, 64)
    v = rt._check_target_indexes([0, 63.0], 2, 64)
    assert v.dtype == np.float32 and v.tolist() == [0.0, 63.0]
    d = rt.default_target_indexes(3, 64)
    assert d.tolist() == [16.0, 32.0, 48.0]
    assert rt.TARGET_MODE_MULTIPLE == 1 and rt.MAX_SOURCES == 8


def test_set_target_indexes_rejects_bad_arguments_before_touching_the_device():
    from gcc_nmf_amd import realtime as rt
    p = object.__new__(rt.GCCNMFProcessor)
    p.device, p._sources, p.numTDOAs = 'cpu', 2, 64
    with pytest.raises(ValueError):
        rt.GCCNMFProcessor.setTargetTDOAIndexes.__wrapped__(p, [1, 2, 3])
    with pytest.raises(ValueError):
        rt.GCCNMFProcessor.setTargetTDOAIndexes.__wrapped__(p, [1, 64])


def test_ctypes_table_is_unchanged():
    """No new entry point: the mode is a frames_mode bit of the existing call."""
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    assert _hip.SIGNATURES['gccnmf_rt_process_block_ll'] == (c_int, [c_void_p] * 23 + [c_int] * 15 + [c_void_p])
    assert _hip.SIGNATURES['gccnmf_rt_process_block'] == (c_int, [c_void_p] * 19 + [c_int] * 13 + [c_void_p])
    assert len(_hip.SIGNATURES) == 46
