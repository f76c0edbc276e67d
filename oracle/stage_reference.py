"""Stage the reference's driver for the drop-in driver tests (tests/test_dropin_cpu.py, tests/test_gpu_pipeline.py).

Copies gccNMF/*.py of an unmodified seanwood/gcc-nmf checkout into oracle/_ref/reference_checkout/gccNMF/ and the driver's
input mixture (the committed tests/golden/data copy) into oracle/_ref/reference_checkout/data/.  oracle/_ref/ is git-ignored,
so nothing of the reference enters the repository; the staged copy travels with the working tree to a machine that has no
checkout of its own.  build() calls stage(); without a checkout it leaves oracle/_ref/ as it is, and the tests skip.

    python oracle/stage_reference.py        # GCCNMF_REFERENCE_ROOT: where the checkout is (same default as make_golden.py)
"""
import glob
import os
import shutil

REF_ROOT = os.environ.get('GCCNMF_REFERENCE_ROOT', '/root/reference')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST = os.path.join(REPO, 'oracle', '_ref', 'reference_checkout')
MIXTURE = 'dev1_female3_liverec_130ms_1m_mix.wav'          # the input runGCCNMF.py reads


def stage(ref_root=REF_ROOT, dst=DST):
    """Returns the staged directory, or None when `ref_root` holds no readable checkout of the reference."""
    sources = sorted(glob.glob(os.path.join(ref_root, 'gccNMF', '*.py')))
    if not os.path.isfile(os.path.join(ref_root, 'gccNMF', 'runGCCNMF.py')) or not all(os.access(f, os.R_OK) for f in sources):
        return None
    os.makedirs(os.path.join(dst, 'gccNMF'), exist_ok=True)
    os.makedirs(os.path.join(dst, 'data'), exist_ok=True)
    for f in sources:
        shutil.copyfile(f, os.path.join(dst, 'gccNMF', os.path.basename(f)))
    shutil.copyfile(os.path.join(REPO, 'tests', 'golden', 'data', MIXTURE), os.path.join(dst, 'data', MIXTURE))
    return dst


if __name__ == '__main__':
    print(stage() or 'no reference checkout at %s: nothing staged' % REF_ROOT)
