"""CPU: the host-side plan of the gather-mode fp32 weight gradient and its refusal of uncovered shapes before any launch."""
import ctypes

import pytest

S1, S2, UP2 = 0, 1, 2
# (B, Cin, Hs, Ws, Cout, mode, taps): the shapes of tests/test_gpu_wgrad_f32_gather.py
COVERED = [(2, 64, 8, 8, 64, S2, 9), (3, 36, 7, 7, 20, S2, 9), (2, 32, 28, 28, 64, S2, 9), (2, 64, 14, 14, 64, S2, 9),
           (2, 64, 16, 32, 64, S2, 9), (5, 64, 32, 32, 128, S2, 9), (2, 72, 16, 16, 136, S2, 9), (2, 64, 64, 64, 64, S2, 9),
           (2, 3, 16, 16, 64, S2, 9), (2, 64, 2, 2, 64, UP2, 9), (3, 36, 7, 7, 20, UP2, 9), (2, 128, 8, 16, 64, UP2, 9),
           (5, 64, 16, 16, 64, UP2, 9), (2, 64, 32, 32, 64, UP2, 9), (2, 3, 16, 16, 64, S1, 9), (2, 64, 16, 16, 3, S1, 9),
           (2, 6, 8, 8, 64, S1, 9), (3, 3, 64, 64, 64, S1, 9), (3, 64, 64, 64, 3, S1, 9), (2, 3, 8, 8, 5, S1, 1)]
# (B, Hs, Ws, Cin, Ho, Wo, Cout, mode, taps): S2 with Wo 64, UP2 with Wo 128, 1x1 at stride 2, Ho that does not follow from Hs, Wo 2
UNCOVERED = [(2, 128, 128, 64, 64, 64, 64, S2, 9), (2, 64, 64, 64, 128, 128, 64, UP2, 9), (2, 16, 16, 64, 8, 8, 64, S2, 1),
             (2, 16, 16, 64, 9, 8, 64, S2, 9), (2, 8, 4, 64, 4, 2, 64, S2, 9)]


def _plan(args):
    from infodiffusion_amd import _lib
    s, n = ctypes.c_int(-1), ctypes.c_long(-1)
    ok = _lib.load().idf_conv_wgrad_f32_gather_plan(*args, ctypes.byref(s), ctypes.byref(n))
    return ok, s.value, n.value


def _args(case):
    B, Cin, Hs, Ws, Cout, mode, taps = case
    Ho, Wo = ((Hs + 1) // 2, (Ws + 1) // 2) if mode == S2 else (2 * Hs, 2 * Ws) if mode == UP2 else (Hs, Ws)
    return B, Hs, Ws, Cin, Ho, Wo, Cout, mode, taps


def test_plan_covers_the_tested_shapes():
    plans = [_plan(_args(c)) for c in COVERED]
    assert all(ok == 1 and s >= 1 for ok, s, _ in plans)
    for (_, Cin, _, _, Cout, _, taps), (_, s, n) in zip(COVERED, plans):
        slab = -(-Cout * taps * Cin // 4) * 4 + -(-Cout // 4) * 4        # dW and db each padded to float4s
        assert n == (s * slab if s > 1 else 0)
    assert any(s == 1 for _, s, _ in plans) and any(s > 1 for _, s, _ in plans)


@pytest.mark.parametrize('args', UNCOVERED)
def test_plan_refuses(args):
    assert _plan(args)[0] == 0


def test_uncovered_shape_is_refused_before_any_launch():
    from infodiffusion_amd import _lib
    lib = _lib.load()
    rc = lib.idf_conv_wgrad_f32_gather(None, None, None, None, None, *UNCOVERED[0], None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert b'conv_wgrad_f32_gather' in lib.idf_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, 'idf_conv_wgrad_f32_gather')
