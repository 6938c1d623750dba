"""The multi-view VAE encoder without a GPU: the C ABI of include/ln3d_encoder.h rejects missing buffers before it launches anything,
the module tree equals the reference's (golden manifest, 11 118 104 parameters), checkpoints load under every encoder prefix, and the
configurations that are not built are refused with a reason."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT, golden, manifest

N = None
I64 = C.c_int64
NULL_CALLS = {
    'ln3d_im2col3x3_pad01': (N, N, 1, 8, 8, 64, 576, N),
    'ln3d_frame_mean': (N, N, 1, 6, 64, 24, N),
    'ln3d_mv_posterior': (N, I64(1536), I64(24), I64(1), N, N, N, N, N, N, N, N, N, 1, 6, 64, 4, N),
}


def test_encoder_entry_points_reject_missing_buffers(hip_lib):
    hdr = open(os.path.join(ROOT, 'include', 'ln3d_encoder.h')).read()
    declared = set(re.findall(r'^int (ln3d_[a-z0-9_]+)\(', hdr, re.M))
    assert declared == set(NULL_CALLS), declared ^ set(NULL_CALLS)
    for name, args in NULL_CALLS.items():
        assert getattr(hip_lib, name)(*args) == -1, name                    # LN3D_ERR_BAD_ARG
    # one real-looking buffer is not enough either: every output of the posterior is required
    fake = C.c_void_p(0x10000)
    assert hip_lib.ln3d_mv_posterior(fake, I64(1536), I64(24), I64(1), fake, fake, N, fake, fake, fake, fake, fake, N, 1, 6, 64, 4, N) == -1
    # shape arguments are validated too (fake, never dereferenced addresses)
    assert hip_lib.ln3d_im2col3x3_pad01(fake, fake, 1, 8, 8, 60, 576, N) == -1               # C % 8
    assert hip_lib.ln3d_im2col3x3_pad01(fake, fake, 1, 1, 8, 64, 576, N) == -1               # H < 2
    assert hip_lib.ln3d_mv_posterior(fake, I64(1536), I64(24), I64(1), fake, fake, N, fake, fake, fake, fake, fake, fake, 1, 6, 64, 3, N) == -1


def _encoder(**kw):
    from ln3diff_amd.vit.mv_encoder import create_encoder
    return create_encoder(**kw)


def test_module_tree_matches_reference_manifest():
    enc = _encoder()
    g = golden('encoder_mv_small')
    mine = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    ref = manifest(g)
    assert mine == ref, set(mine) ^ set(ref)
    assert sum(v.numel() for v in enc.state_dict().values()) == int(g['n_params']) == 11118104


@pytest.mark.parametrize('prefix', ['rec_model.encoder.', 'auto_encoder.encoder.', 'encoder.', 'module.encoder.'])
def test_load_checkpoint_encoder_prefixes(tmp_path, prefix):
    from ln3diff_amd.checkpoint import load_checkpoint
    from ln3diff_amd.synth import synth_state_dict
    enc = _encoder()
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    sd = synth_state_dict(shapes, 3)
    path = tmp_path / 'vae.pt'
    torch.save({prefix + k: v for k, v in sd.items()}, path)
    rep = load_checkpoint(str(path), encoder=enc)
    assert rep['encoder'] == {prefix: len(sd)}
    for k, v in enc.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # a file without encoder tensors: skip_absent reports it, strict loading raises
    torch.save({'decoder.x': torch.zeros(1)}, tmp_path / 'other.pt')
    assert load_checkpoint(str(tmp_path / 'other.pt'), encoder=enc, skip_absent=True)['encoder'] == 'absent'
    with pytest.raises(RuntimeError):
        load_checkpoint(str(tmp_path / 'other.pt'), encoder=enc)


def test_unbuilt_configurations_are_refused():
    from ln3diff_amd.vit.mv_encoder import MVEncoderGSDynamicInp, create_encoder
    from ln3diff_amd.nsr.script_util import AE
    with pytest.raises(NotImplementedError, match='dino_version'):
        create_encoder(dino_version='mv-sd-dit')                 # the 4-view MVEncoder with its fusion layer
    with pytest.raises(NotImplementedError):
        create_encoder(dino_version='sd-dit')
    with pytest.raises(ValueError, match='num_frames'):
        create_encoder(num_frames=4)
    enc = create_encoder()
    with pytest.raises(ValueError, match='num_frames'):
        enc(torch.zeros(6, 10, 64, 64), num_frames=3)
    with pytest.raises(ValueError, match='multiple of num_frames'):
        enc(torch.zeros(7, 10, 64, 64))
    with pytest.raises(ValueError, match='multiple of num_frames'):
        enc.forward_frames(torch.zeros(8, 10, 64, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        enc.forward_frames(torch.zeros(6, 10, 64, 64))
    with pytest.raises(NotImplementedError, match='dino_version'):
        AE(enc, None, 128, dino_version='sd_dit')
    with pytest.raises(NotImplementedError):
        MVEncoderGSDynamicInp(ch=64, out_ch=3, ch_mult=[1, 2, 4, 4], num_res_blocks=1, attn_resolutions=[32], in_channels=10,
                              resolution=256, z_channels=12, num_frames=6, attn_kwargs={'n_heads': 8, 'd_head': 64})
    ae = AE(None, None, 128)                                      # the sampling configuration keeps refusing the encoder behaviours
    for b in ('enc', 'enc_dec', 'encoder_vae', 'dec', 'dec_wo_triplane', 'enc_dec_wo_triplane'):
        with pytest.raises(NotImplementedError):
            ae(img=torch.zeros(6, 10, 64, 64), behaviour=b)
