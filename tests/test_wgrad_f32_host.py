"""CPU: the host-side plan of the fp32 ordered-slab weight gradient and its refusal of uncovered shapes before any launch."""
import ctypes

import pytest

# (B, H, W, Cin, Cout, taps): the shapes of tests/test_gpu_wgrad_f32.py
COVERED = [(2, 4, 4, 64, 64, 9), (3, 7, 7, 36, 20, 9), (2, 8, 16, 64, 64, 9), (2, 16, 8, 64, 64, 9), (2, 28, 28, 32, 64, 9),
           (2, 14, 14, 32, 64, 9), (2, 16, 16, 72, 136, 9), (5, 32, 32, 64, 64, 9), (3, 64, 64, 64, 64, 9), (2, 8, 8, 256, 256, 9),
           (2, 16, 16, 64, 72, 1), (3, 16, 16, 256, 256, 1), (2, 64, 64, 64, 64, 1)]
# Cin 3, Cout 3, Cin 6, W 128, W 2
UNCOVERED = [(2, 16, 16, 3, 64, 9), (2, 16, 16, 64, 3, 9), (2, 16, 16, 6, 64, 9), (2, 128, 128, 64, 64, 9), (2, 8, 2, 64, 64, 9)]


def _plan(shape):
    from infodiffusion_amd import _lib
    s, n = ctypes.c_int(-1), ctypes.c_long(-1)
    ok = _lib.load().idf_conv_wgrad_f32_plan(*shape, ctypes.byref(s), ctypes.byref(n))
    return ok, s.value, n.value


def test_plan_covers_the_tested_shapes():
    plans = [_plan(c) for c in COVERED]
    assert all(ok == 1 and s >= 1 for ok, s, _ in plans)
    for (B, H, W, Cin, Cout, taps), (_, s, n) in zip(COVERED, plans):
        assert n == (s * (Cout * taps * Cin + Cout) if s > 1 else 0)      # a multiple of 4 floats as it stands
    assert any(s == 1 for _, s, _ in plans) and any(s > 1 for _, s, _ in plans)


@pytest.mark.parametrize('shape', UNCOVERED)
def test_plan_refuses(shape):
    assert _plan(shape)[0] == 0


def test_uncovered_shape_is_refused_before_any_launch():
    from infodiffusion_amd import _lib
    lib = _lib.load()
    rc = lib.idf_conv_wgrad_f32(None, None, None, None, None, 2, 16, 16, 3, 64, 9, None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert b'conv_wgrad_f32' in lib.idf_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, 'idf_conv_wgrad_f32')
