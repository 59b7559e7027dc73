"""CPU: the host-side predicate of the fp32 DownSample / UpSample convs (idf_conv_resample_f32) and its refusal of uncovered
shapes before any launch.  Shapes are (B, Hs, Ws, Cin, Cout) of the forward conv; ops 0 .. 3 = S2 forward, S2 data
gradient, UP2 forward, UP2 data gradient."""
import pytest

# (B, K, H, W, N) over the low-resolution map, as tests/test_gpu_conv_resample_f32.py: (K, N) = (Cin, Cout) forward, (Cout, Cin) data gradient
LOW = [(2, 32, 4, 4, 64), (3, 32, 5, 6, 32), (2, 64, 8, 16, 20), (2, 64, 16, 8, 72), (2, 96, 8, 8, 64), (2, 32, 10, 16, 32),
       (2, 64, 32, 32, 128), (32, 128, 8, 8, 128), (16, 64, 32, 32, 64), (32, 64, 32, 32, 64)]
COVERED = [((B, H * (1 if op >= 2 else 2), W * (1 if op >= 2 else 2), *((N, K) if op & 1 else (K, N))), op)
           for B, K, H, W, N in LOW for op in range(4)]
COVERED.append(((2, 9, 11, 32, 32), 0))          # S2 forward from an odd map
# measured out: S2 forward launches that fill the chip, the UP2 data gradient of the 8 x 8 map at the training batch
GATED = [((16, 64, 64, 64, 64), 0), ((32, 64, 64, 64, 64), 0), ((32, 8, 8, 128, 128), 3)]
COVERED = [c for c in COVERED if c not in GATED]
REFUSED = [((2, 16, 16, 3, 64), 0), ((2, 16, 16, 3, 64), 2), ((2, 16, 16, 64, 3), 1), ((2, 16, 16, 64, 3), 3),    # K side 3
           ((2, 16, 16, 48, 64), 0), ((2, 16, 16, 64, 48), 3),                                                  # K side 48
           ((2, 8, 4, 64, 64), 0), ((2, 8, 2, 64, 64), 2),                                                      # width 2
           ((2, 256, 256, 64, 64), 1), ((2, 128, 128, 64, 64), 3),                                              # width 128
           ((2, 9, 16, 64, 64), 1),                                                                             # odd Hs, S2 dgrad
           ((2, 16, 16, 64, 64), 4)]                                                                            # no such op


@pytest.mark.parametrize('shape,op', COVERED + REFUSED + GATED)
def test_predicate(shape, op):
    from infodiffusion_amd import _lib
    assert _lib.load().idf_conv_resample_f32_ok(*shape, op) == (1 if (shape, op) in COVERED else 0)


def test_uncovered_shape_is_refused_before_any_launch():
    from infodiffusion_amd import _lib
    lib = _lib.load()
    rc = lib.idf_conv_resample_f32(None, None, None, None, None, 2, 16, 16, 3, 64, 0, None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert b'conv_resample_f32' in lib.idf_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, 'idf_conv_resample_f32')
