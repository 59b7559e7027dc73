"""CPU: the host-side predicate of the split-bf16 fp32 attention (idf_attn_f32_split_ok) and the refusal of uncovered shapes
before any launch.  Shapes are (B, N, D, terms)."""
import pytest

COVERED = [(B, N, D, t) for B in (0, 1, 3, 32, 127, 128, 512) for N in (64, 256) for D in (64, 128) for t in (2, 3)]
REFUSED = [(2, 128, 128, 3), (2, 256, 96, 3), (2, 256, 128, 1), (2, 256, 128, 4), (2, 64, 64, 0), (-1, 256, 128, 3)]


@pytest.mark.parametrize('shape', COVERED + REFUSED)
def test_predicate(shape):
    from infodiffusion_amd import _lib
    assert _lib.load().idf_attn_f32_split_ok(*shape) == (1 if shape in COVERED else 0)


def test_exact_kernel_gate_is_unchanged():
    from infodiffusion_amd import _lib
    assert _lib.load().idf_attn_f32_ok(32, 256, 128) == 0


@pytest.mark.parametrize('entry,nptr', [('idf_attn_f32_split_fwd', 3), ('idf_attn_f32_split_bwd', 5)])
def test_uncovered_shape_is_refused_before_any_launch(entry, nptr):
    from infodiffusion_amd import _lib
    lib = _lib.load()
    for shape_terms in ((2, 128, 96, 3), (2, 256, 128, 4)):
        rc = getattr(lib, entry)(*[None] * nptr, *shape_terms[:3], 128 ** -0.5, shape_terms[3], None)
        assert rc == _lib.ERR_UNSUPPORTED
        assert entry.encode() in lib.idf_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, entry)
    assert getattr(lib, entry)(*[None] * nptr, 2, 64, 128, 128 ** -0.5, 3, None) == _lib.ERR_BADARG     # covered shape, null operands
