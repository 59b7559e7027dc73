"""CPU: the host-side predicate and shadow size of the split-bf16 3x3 conv, and run.py's --f32_mfma flag."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERED = [(2, 4, 4, 32, 64), (2, 16, 16, 64, 3), (2, 16, 16, 64, 72), (3, 64, 64, 64, 64), (32, 64, 64, 32, 64)]
# Cin = 48, W = 2, W = 128
UNCOVERED = [(2, 16, 16, 48, 64), (2, 8, 2, 64, 64), (2, 128, 128, 64, 64)]


@pytest.mark.parametrize('terms', [1, 2, 3, 4])
@pytest.mark.parametrize('shape', COVERED + UNCOVERED)
def test_predicate(shape, terms):
    from infodiffusion_amd import _lib
    lib = _lib.load()
    ok = shape in COVERED and terms in (2, 3)
    assert lib.idf_conv3x3_f32_split_ok(*shape, terms) == (1 if ok else 0)     # (B, H, W, Cin, Cout, terms)
    if not ok:          # refused before any launch
        assert lib.idf_conv3x3_f32_split(None, None, None, None, None, *shape, terms, None) == _lib.ERR_UNSUPPORTED
        assert b'conv3x3_f32_split' in lib.idf_last_error()


@pytest.mark.parametrize('rows,Cin,terms', [(64, 32, 3), (3, 64, 2), (72, 192, 3), (16, 32, 2)])
def test_split_weight_bytes(rows, Cin, terms):
    from infodiffusion_amd import _lib
    assert _lib.load().idf_split_weight_bytes(rows, 9, Cin, terms) == -(-rows // 16) * 16 * 9 * Cin * 2 * terms


def test_run_py_refuses_split_mode_with_bf16_activations():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), '--model', 'diff', '--mode', 'train', '--prior', 'regular',
                        '--dataset', 'celeba', '--a_dim', '32', '--f32_mfma', 'bf16x3', '--act_dtype', 'bf16'],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and '--f32_mfma' in r.stderr
