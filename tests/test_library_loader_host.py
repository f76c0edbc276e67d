"""CPU-only: the one loader of the four ctypes bindings (``_hip.load_library``) as each module's ``lib()`` reaches it.  A missing file and a
missing symbol are errors with the texts the modules have always had; only ``lenient`` (the GCCNMF_HIP_LIB rule of ``_hip.lib()``) skips a
missing symbol."""
import ctypes
import importlib

import pytest

MODULES = ['_hip', '_array', '_array_spatial', '_eval']
ABSENT = 'gccnmf_no_such_entry_point'


@pytest.fixture(params=MODULES)
def binding(request, monkeypatch):
    mod = importlib.import_module('gcc_nmf_amd.' + request.param)
    monkeypatch.setattr(mod, '_lib', None)                     # (restored afterwards: a loaded handle stays loaded)
    monkeypatch.delenv('GCCNMF_HIP_LIB', raising=False)
    monkeypatch.delenv('GCCNMF_TUNE', raising=False)
    return mod


def test_a_missing_library_is_an_error_that_says_how_to_build_it(binding, monkeypatch, tmp_path):
    from gcc_nmf_amd._hip import HipLibraryError
    path = str(tmp_path / 'libgccnmf_absent.so')
    monkeypatch.setattr(binding, 'LIB_PATH', path)
    with pytest.raises(HipLibraryError) as e:
        binding.lib()
    assert path in str(e.value) and 'is missing' in str(e.value) and '`make -C gcc_nmf_amd/csrc`' in str(e.value)
    assert 'no CPU fallback' in str(e.value) and binding._lib is None


def test_a_missing_symbol_is_an_error_that_names_it(binding, monkeypatch):
    from gcc_nmf_amd._hip import HipLibraryError
    monkeypatch.setattr(binding, 'SIGNATURES', dict(binding.SIGNATURES, **{ABSENT: (ctypes.c_int, [])}))
    with pytest.raises(HipLibraryError) as e:
        binding.lib()
    assert '%s does not export %s' % (binding.LIB_PATH, ABSENT) in str(e.value) and 're-run make -C gcc_nmf_amd/csrc' in str(e.value)
    assert binding._lib is None


def test_lenient_skips_a_missing_symbol_and_types_the_rest():
    from gcc_nmf_amd import _hip
    signatures = dict(_hip.SIGNATURES, **{ABSENT: (ctypes.c_int, [])})
    with pytest.raises(_hip.HipLibraryError):
        _hip.load_library(_hip.LIB_PATH, signatures)
    handle = _hip.load_library(_hip.LIB_PATH, signatures, optional={ABSENT + '_2': (ctypes.c_int, [])}, lenient=True)
    assert not hasattr(handle, ABSENT) and not hasattr(handle, ABSENT + '_2')
    for name, (restype, argtypes) in _hip.SIGNATURES.items():
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
