"""FFHQ VAE decoder class (vit/vit_triplane_ffhq.py): module tree, launcher wiring, preset, checkpoint loading and the argument
checks of its fused roll-out convolution, without a GPU."""
import ctypes
import json
import os
import shlex

import numpy as np
import pytest
import torch

from ln3diff_amd.entry import create_argparser, validate
from ln3diff_amd.nsr.triplane import Triplane
from ln3diff_amd.vit import vit_triplane_ffhq as ffhq

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
CLASS = 'vit.vit_triplane.' + ffhq.CLASS_NAME
FFHQDec = getattr(ffhq, ffhq.CLASS_NAME)

# the flags of shell_scripts/final_release/inference/sample_ffhq_t23d.sh, verbatim and in its order (variables expanded)
LAUNCHER = ("--num_workers 4 --depth_lambda 0 "
            "--iterations 10001 --anneal_lr False --batch_size 1 --save_interval 10000 --image_size_encoder 224 --image_size 128 "
            "--dino_version v2 --sr_training False --cls_token False --weight_decay 0.05 --image_size 128 --kl_lambda 0 "
            "--no_dim_up_mlp True --uvit_skip_encoder True --fg_mse True --bg_lamdba 0.01 "
            "--decoder_in_chans 32 --out_chans 96 --alpha_lambda 1 --logdir ./logs/ffhq --arch_encoder vits --arch_decoder vitb "
            "--vit_decoder_wd 0.001 --encoder_weight_decay 0.001 --color_criterion mse --triplane_in_chans 32 --decoder_output_dim 32 "
            "--ae_classname " + CLASS + " "
            "--diffusion_steps 1000 --noise_schedule linear --use_kl False --use_amp False --triplane_scaling_divider 1 "
            "--trainer_name vpsde_crossattn --mixed_prediction True --denoise_in_channels 12 --denoise_out_channels 12 "
            "--diffusion_input_size 32 --p_rendering_loss False --pred_type v --predict_v True "
            "--train_vae False --create_controlnet False --control_key img_sr "
            "--learn_sigma False --num_heads 8 --num_res_blocks 2 --num_channels 320 --attention_resolutions 4,2,1 "
            "--use_spatial_transformer True --transformer_depth 1 --context_dim 768 "
            "--data_dir /mnt/yslan/datasets/cache/lmdb_debug/ffhq "
            "--resume_checkpoint checkpoints/ffhq/model_joint_denoise_rec_model1580000.pt "
            "--encoder_lr 1e-5 --vit_decoder_lr 1e-5 --triplane_decoder_lr 0.0005 --super_resolution_lr 0.0005 --lr 2e-5 "
            "--lpips_lambda 0.8 --overfitting False --load_pretrain_encoder True --iterations 5000001 --save_interval 10000 "
            "--eval_interval 2500 --decomposed True --logdir ./logs/ffhq --cfg ffhq --patch_size 14 --eval_batch_size 1 "
            "--prompt 'a middle aged woman with brown hair, wearing glasses.' --interval 5 --save_img True --num_samples 1 "
            "--use_train_trajectory False --normalize_clip_encoding True --scale_clip_encoding 18.4 --overwrite_diff_inp_size 16 "
            "--use_lmdb True --timestep_respacing ddim250 --use_ddim True --unconditional_guidance_scale 6.5")


def _args(flags):
    return create_argparser(False).parse_known_args(shlex.split(flags))[0]


def _build(D=128, heads=2):
    tp = Triplane(img_resolution=128, rendering_kwargs=ffhq.ffhq_rendering_kwargs('ffhq'), decoder_output_dim=32)
    return FFHQDec(ffhq.DinoVisionTransformer(D, 12, heads), tp, False)


def test_validate_accepts_the_ffhq_launcher():
    a = _args(LAUNCHER)
    assert a.ae_classname == CLASS and a.create_dit is False and a.cfg == 'ffhq' and a.overwrite_diff_inp_size == '16'
    assert validate(a) == 'gd'


@pytest.mark.parametrize('tag', ['ffhq_dec_small', 'ffhq_dec_released'])
def test_state_dict_manifest_matches_the_reference_class(tag):
    g = np.load(os.path.join(GOLDEN, tag + '.npz'))
    ref = json.loads(g['manifest'].tobytes().decode())
    D = 128 if 'small' in tag else 768
    own = {k: list(v.shape) for k, v in _build(D, 2 if D == 128 else 12).state_dict().items()}
    assert own == ref
    if 'n_params' in g:
        assert sum(int(np.prod(s)) for s in own.values()) == int(g['n_params'])


def test_class_is_reachable_by_its_launcher_name():
    from ln3diff_amd.vit import vit_triplane
    assert getattr(vit_triplane, ffhq.CLASS_NAME) is FFHQDec


def test_cfg_ffhq_gives_the_reference_rendering_kwargs():
    with open(os.path.join(GOLDEN, 'ffhq_rendering_kwargs.json')) as f:
        fx = json.load(f)
    assert fx['flags'] == {'cfg': 'ffhq'}
    rk = json.loads(json.dumps(ffhq.ffhq_rendering_kwargs('ffhq')))
    ref = dict(fx['rendering_kwargs'])
    # the package's one documented difference (nsr/triplane.py OBJAVERSE_RENDERING_KWARGS): the per-sample tensors are opt-in
    assert ref.pop('return_sampling_details_flag') is True and rk.pop('return_sampling_details_flag') is False
    assert rk == ref
    assert (rk['depth_resolution'], rk['depth_resolution_importance'], rk['ray_start'], rk['ray_end'], rk['box_warp']) == (48, 48, 2.25, 3.3, 1)
    assert _build().rendering_kwargs['ray_end'] == 3.3


def test_ffhq_class_refuses_unknown_cfg_other_engines_and_other_latents():
    with pytest.raises(SystemExit) as e:
        validate(_args(LAUNCHER.replace('--cfg ffhq', '--cfg ffhq_512')))
    assert 'ffhq_512' in str(e.value)
    with pytest.raises(SystemExit) as e:
        validate(create_argparser(True).parse_known_args(["--ae_classname", CLASS])[0])       # the DiT / sgm path
    assert 'FFHQ decoder class' in str(e.value)
    with pytest.raises(SystemExit):
        validate(_args(LAUNCHER + " --create_dit true"))                                      # a DiT under the gd engines
    with pytest.raises(SystemExit) as e:
        validate(_args(LAUNCHER.replace('--overwrite_diff_inp_size 16', '')))                 # a 32 x 32 latent
    assert '16' in str(e.value)
    with pytest.raises(SystemExit) as e:
        validate(_args(LAUNCHER.replace(CLASS, CLASS + '_v2')))
    assert 'released decoder class' in str(e.value)


def test_encoder_behaviours_are_refused():
    dec = _build()
    x = torch.zeros(1, 256, 384)
    for call in (lambda: dec.vae_reparameterization(x, False), lambda: dec.vit_decode(x, 128), lambda: dec.vae_encode(x)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(RuntimeError):                   # decoding is HIP only: no CPU fall-back
        dec.vit_decode_backbone(torch.zeros(1, 12, 16, 16))


def test_checkpoint_round_trip(tmp_path):
    from ln3diff_amd.checkpoint import load_checkpoint
    from ln3diff_amd.synth import synth_vit_state_dict
    src = _build()
    sd = synth_vit_state_dict({k: tuple(v.shape) for k, v in src.state_dict().items()}, 3)
    path = tmp_path / 'model_joint_denoise_rec_model.pt'
    torch.save({'rec_model.decoder.' + k: v for k, v in sd.items()}, path)
    dst = _build()
    rep = load_checkpoint(str(path), decoder=dst)
    assert rep['decoder'] == {'rec_model.decoder.': len(sd)}
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_fused_conv_checks_its_arguments():
    """ln3d_conv3x3_rollout_bf16 validates before it touches the device: null pointers, C % 16 != 0 (one MFMA K step is 16 channels),
    C > 128 (the LDS tile), Cout % 32 != 0 and out == x return LN3D_ERR_BAD_ARG (-1)."""
    from ln3diff_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libln3d_hip.so not built')
    L = _lib.lib()
    for s in ('ln3d_conv3x3_rollout_bf16', 'ln3d_rollout_means_bf16'):
        assert hasattr(L, s)
    buf = (ctypes.c_float * 16)()
    buf2 = (ctypes.c_float * 16)()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)

    def call(ptrs=None, H=8, W=8, C=32, Cout=32, out=q):
        a = ptrs or [p] * 6
        return L.ln3d_conv3x3_rollout_bf16(a[0], 0, a[1], a[2], a[3], a[4], a[5], H, W, out, H, W, C, Cout, ctypes.c_float(0.01), None)
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert call(ptrs) == -1
    assert call(out=None) == -1
    assert call(C=24) == -1 and call(C=8) == -1 and call(C=144) == -1 and call(Cout=48) == -1 and call(H=0) == -1
    assert call(out=p) == -1                                            # out must not be x
    assert L.ln3d_rollout_means_bf16(None, p, p, 3, 8, 8, 32, None) == -1
