"""CPU: the host-side predicate of the fp32 halo-tile 3x3 conv and its refusal of uncovered shapes before any launch."""
import pytest

COVERED = [(2, 4, 4, 32, 64), (2, 8, 16, 64, 64), (2, 16, 8, 64, 64), (3, 7, 7, 32, 32), (2, 28, 28, 32, 64),
           (2, 16, 16, 64, 3), (2, 16, 16, 64, 72), (2, 8, 8, 192, 64), (3, 64, 64, 64, 64), (2, 32, 32, 256, 128),
           (2, 14, 14, 64, 64), (2, 10, 20, 32, 32), (32, 64, 64, 32, 64), (3, 64, 64, 32, 3), (32, 64, 64, 32, 3)]
# Cin = 3, Cin = 48, W = 128, W = 2
UNCOVERED = [(2, 16, 16, 3, 64), (2, 16, 16, 48, 64), (2, 128, 128, 64, 64), (2, 8, 2, 64, 64)]


@pytest.mark.parametrize('shape', COVERED + UNCOVERED)
def test_predicate(shape):
    from infodiffusion_amd import _lib
    assert _lib.load().idf_conv3x3_f32_ok(*shape) == (1 if shape in COVERED else 0)     # (B, H, W, Cin, Cout)


def test_uncovered_shape_is_refused_before_any_launch():
    from infodiffusion_amd import _lib
    lib = _lib.load()
    rc = lib.idf_conv3x3_f32(None, None, None, None, None, 2, 16, 16, 3, 64, None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert b'conv3x3_f32' in lib.idf_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, 'idf_conv3x3_f32')
