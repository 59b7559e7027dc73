"""CPU: the C-ABI library builds, loads, and exports every symbol include/infodiff_hip.h
declares (no compute calls without a GPU); the product refuses to run without it."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, 'include', 'infodiff_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(idf_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    from infodiffusion_amd import build, _lib
    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), 'missing export: ' + n
    # the ctypes table binds exactly the declared entry points
    assert sorted(_lib.SIGNATURES) == names
    _lib.load()
    assert _lib.load().idf_version() >= 100
    assert _lib.load().idf_last_error() is not None


def test_error_channel_without_gpu():
    from infodiffusion_amd import _lib
    lib = _lib.load()
    rc = lib.idf_sampler_step(None, None, None, None, None, None, None, 7, 0, 0, None)   # bad mode: rejected before any launch
    assert rc == _lib.ERR_BADARG
    assert b'bad mode' in lib.idf_last_error()
    with pytest.raises(_lib.HipKernelError):
        _lib.check(rc, 'idf_sampler_step')


def test_missing_library_fails_loudly(monkeypatch):
    from infodiffusion_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libinfodiff_hip.so')
    with pytest.raises(ImportError):
        _lib.load()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'infodiffusion_amd')
    for fn in os.listdir(pkg):
        if fn.endswith('.py'):
            assert 'oracle' not in open(os.path.join(pkg, fn)).read().replace('no oracle', ''), fn


def test_state_dict_matches_reference_manifest():
    import json
    import types
    import torch
    from infodiffusion_amd.models import InfoDiff
    args = types.SimpleNamespace(beta1=1e-5, betaT=1e-2, diffusion_steps=1000, input_size=64, is_bottleneck=False,
                                 unets_channels=64, encoder_channels=64, a_dim=32, mmd_weight=0.1, kld_weight=0.0)
    m = InfoDiff(args, 'cpu', (3, 64, 64))
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'manifest_celeba.json')))
    sd = m.state_dict()
    assert [k for k, _ in man] == list(sd.keys())
    assert all(tuple(s) == tuple(sd[k].shape) for k, s in man)
    assert len(sd) == 969


def test_checkpoint_interchange_with_reference(manifest):
    """state_dicts load strictly in both directions and seeded init is bit-identical -- against the record the
    reference's own InfoDiff left of its state_dict under the same seed (tools/gen_golden.py ckpt_init -> tests/golden/
    ckpt_init_seed3.json: key, shape, dtype and SHA-256 of every entry, in order)."""
    import hashlib
    import types
    import torch
    from infodiffusion_amd.models import InfoDiff
    args = types.SimpleNamespace(beta1=1e-5, betaT=1e-2, diffusion_steps=100, input_size=32, is_bottleneck=False,
                                 unets_channels=32, encoder_channels=32, a_dim=16, mmd_weight=0.1, kld_weight=0.0)
    torch.manual_seed(3)
    ours = InfoDiff(args, 'cpu', (1, 32, 32))
    so, ref = ours.state_dict(), manifest('ckpt_init_seed3')
    assert len(ref) > 100
    # what a strict load needs in either direction: the same keys in the same order, entry for entry the same shape and dtype
    assert list(so) == [k for k, _, _, _ in ref]
    assert all(list(so[k].shape) == s and str(so[k].dtype) == d for k, s, d, _ in ref)
    # same seed -> same weights, bit for bit
    for k, _, _, h in ref:
        assert hashlib.sha256(so[k].contiguous().numpy().tobytes()).hexdigest() == h, k
    import io
    buf = io.BytesIO()
    torch.save(so, buf)                                       # run.py:157 format
    buf.seek(0)
    back = torch.load(buf)
    assert all(hashlib.sha256(back[k].contiguous().numpy().tobytes()).hexdigest() == h for k, _, _, h in ref)
    # a check-point laid out as the reference writes it (its keys, shapes and dtypes, dense NCHW tensors), other values
    theirs = {k: (back[k].contiguous() + 1).to(getattr(torch, d.split('.')[1])) for k, _, d, _ in ref}
    ours.load_state_dict(theirs, strict=True)
    assert all(torch.equal(ours.state_dict()[k], theirs[k]) for k in so)
    # conv masters keep their channels-last memory after loading
    assert ours.backbone.downblocks[0].block1[2].weight.stride()[1] == 1


def test_library_sources_issue_kernel_launches_only():
    """Boundary rule: no allocation, synchronisation, memset or memcpy API call inside the library --
    a hipMemsetAsync recorded into a training hipGraph once left a gradient buffer uncleared on replay."""
    import glob
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'infodiffusion_amd', 'csrc')
    banned = re.compile(r'\b(hipMemset\w*|hipMemcpy\w*|hipMalloc\w*|hipFree\w*|hipDeviceSynchronize|hipStreamSynchronize)\s*\(')
    hits = []
    for path in sorted(glob.glob(os.path.join(root, '*'))):
        for n, line in enumerate(open(path, errors='replace'), 1):
            code = line.split('//')[0]
            if banned.search(code):
                hits.append('%s:%d %s' % (os.path.basename(path), n, line.strip()))
    assert not hits, hits
