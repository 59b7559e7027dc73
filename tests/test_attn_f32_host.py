"""CPU: the host-side predicate of the fused fp32 attention (idf_attn_f32_ok) and the refusal of uncovered shapes before any
launch.  Shapes are (B, N, D)."""
import pytest

COVERED = [(B, N, D) for B in (0, 1, 3, 32, 127, 128, 512) for N in (64, 256) for D in (64, 128)]
# rows the performance gate took out of the predicate (profiles/f32_attn.txt): 256 tokens x 128 channels below B = 128
GATED = [(B, 256, 128) for B in (1, 3, 32, 127)]
REFUSED = [(2, N, 128) for N in (16, 49, 128, 1024)] + [(2, 256, D) for D in (32, 96, 256)] + [(-1, 256, 128)]


@pytest.mark.parametrize('shape', COVERED + REFUSED + GATED)
def test_predicate(shape):
    from infodiffusion_amd import _lib
    assert _lib.load().idf_attn_f32_ok(*shape) == (1 if shape in COVERED and shape not in GATED else 0)


@pytest.mark.parametrize('entry,nptr', [('idf_attn_f32_fwd', 3), ('idf_attn_f32_bwd', 5)])
def test_uncovered_shape_is_refused_before_any_launch(entry, nptr):
    from infodiffusion_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, entry)(*[None] * nptr, 2, 49, 128, 128 ** -0.5, None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert entry.encode() in lib.idf_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, entry)
    assert getattr(lib, entry)(*[None] * nptr, 2, 64, 128, 128 ** -0.5, None) == _lib.ERR_BADARG     # covered shape, null operands
