"""CPU: the host-side plan of the split-bf16 fp32 weight gradient (idf_conv_wgrad_f32_split_plan) and its refusal before any launch."""
import ctypes

import pytest

# (B, H, W, Cin, Cout, taps)
COVERED = [(2, 4, 4, 64, 64, 9), (3, 7, 7, 40, 24, 9), (2, 16, 16, 72, 136, 9), (5, 32, 32, 64, 64, 9), (3, 64, 64, 64, 64, 9),
           (2, 16, 16, 64, 72, 1)]
# channel counts that are no multiples of 8, W = 2, W = 128, H = 2, taps 4
UNCOVERED = [(3, 7, 7, 36, 20, 9), (2, 8, 2, 64, 64, 9), (2, 128, 128, 64, 64, 9), (2, 2, 16, 64, 64, 9), (2, 16, 16, 64, 64, 4)]


@pytest.mark.parametrize('terms', [1, 2, 3, 4])
@pytest.mark.parametrize('shape', COVERED + UNCOVERED)
def test_plan(shape, terms):
    from infodiffusion_amd import _lib
    lib = _lib.load()
    B, H, W, Cin, Cout, taps = shape
    s, n = ctypes.c_int(-1), ctypes.c_long(-1)
    ok = shape in COVERED and terms in (2, 3)
    assert lib.idf_conv_wgrad_f32_split_plan(*shape, terms, ctypes.byref(s), ctypes.byref(n)) == (1 if ok else 0)
    if ok:
        assert s.value >= 1 and n.value == (s.value * (Cout * taps * Cin + Cout) if s.value > 1 else 0)
    else:               # refused before any launch
        assert lib.idf_conv_wgrad_f32_split(None, None, None, None, None, *shape, terms, None) == _lib.ERR_UNSUPPORTED
        assert b'conv_wgrad_f32_split' in lib.idf_last_error()
