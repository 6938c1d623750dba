"""ShapeNet VAE decoder class (vit/vit_triplane_shapenet.py): module tree, launcher wiring and checkpoint loading, without a GPU."""
import json
import os
import shlex

import numpy as np
import pytest
import torch

from ln3diff_amd.entry import create_argparser, validate
from ln3diff_amd.nsr.triplane import Triplane
from ln3diff_amd.vit.vit_triplane_shapenet import (RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn as ShapeNetDec, DinoVisionTransformer,
                                                   shapenet_rendering_kwargs)

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
CLASS = 'vit.vit_triplane.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn'

# the model / sampling flags of shell_scripts/final_release/inference/sample_shapenet_{car,chair,plane}_t23d.sh, verbatim (they differ
# only in data paths, checkpoints and prompts)
_COMMON = ("--image_size 128 --image_size_encoder 224 --dino_version v2 --sr_training False --cls_token False --weight_decay 0.05 "
           "--kl_lambda 0 --no_dim_up_mlp True --uvit_skip_encoder True --fg_mse True --vae_p 2 --bg_lamdba 0.01 "
           "--decoder_in_chans 32 --out_chans 96 --alpha_lambda 1 --arch_encoder vits --arch_decoder vitb --vit_decoder_wd 0.001 "
           "--encoder_weight_decay 0.001 --color_criterion mse --decoder_output_dim 32 --ae_classname " + CLASS + " "
           "--diffusion_steps 1000 --noise_schedule linear --use_kl False --use_amp False --triplane_scaling_divider 1 "
           "--trainer_name vpsde_crossattn --mixed_prediction True --denoise_in_channels 12 --denoise_out_channels 12 "
           "--diffusion_input_size 32 --p_rendering_loss False --pred_type v --predict_v True --timestep_respacing ddim250 --use_ddim True "
           "--unconditional_guidance_scale 1.0 --train_vae False --create_controlnet False --control_key img_sr "
           "--learn_sigma False --num_heads 8 --num_res_blocks 2 --num_channels 320 --attention_resolutions 4,2,1 "
           "--use_spatial_transformer True --transformer_depth 1 --context_dim 768 --num_workers 4 --depth_lambda 0 --overfitting False "
           "--load_pretrain_encoder True --iterations 5000001 --save_interval 10000 --eval_interval 2500 --decomposed True "
           "--cfg shapenet_tuneray_aug_resolution_64_64_nearestSR --ray_start 0.6 --ray_end 1.8 --patch_size 14 --eval_batch_size 4 "
           "--interval 5 --save_img True --num_samples 40 --use_train_trajectory False --normalize_clip_encoding True --export_mesh True "
           "--scale_clip_encoding 18.4")
LAUNCHERS = {
    'car': "--logdir ./logs/car --batch_size 4 --prompt 'a SUV car' --resume_checkpoint checkpoints/shapenet/car/model_joint_denoise_rec_model1700000.pt",
    'chair': "--logdir ./logs/chair --batch_size 4 --prompt 'a chair' --resume_checkpoint checkpoints/shapenet/chair/model_joint_denoise_rec_model2070000.pt",
    'plane': "--logdir ./logs/plane --batch_size 4 --prompt 'a plane' --resume_checkpoint checkpoints/shapenet/plane/model_joint_denoise_rec_model770000.pt",
}


def _args(flags):
    return create_argparser(False).parse_known_args(shlex.split(flags))[0]


def _build(D=128, heads=2):
    tp = Triplane(img_resolution=128, rendering_kwargs=shapenet_rendering_kwargs('shapenet_tuneray_aug_resolution_64_64_nearestSR', 0.6, 1.8),
                  decoder_output_dim=32)
    return ShapeNetDec(DinoVisionTransformer(D, 12, heads), tp, False)


@pytest.mark.parametrize('tag', ['shapenet_dec_small', 'shapenet_dec_released'])
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
    assert vit_triplane.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn is ShapeNetDec


@pytest.mark.parametrize('obj', sorted(LAUNCHERS))
def test_validate_accepts_the_shapenet_launchers_and_honours_cfg(obj):
    a = _args(_COMMON + " " + LAUNCHERS[obj])
    assert a.ae_classname == CLASS and a.create_dit is False
    assert validate(a) == 'gd'
    with open(os.path.join(GOLDEN, 'shapenet_rendering_kwargs.json')) as f:
        fx = json.load(f)
    assert fx['flags'] == {'cfg': a.cfg, 'ray_start': a.ray_start, 'ray_end': a.ray_end}
    rk = json.loads(json.dumps(shapenet_rendering_kwargs(a.cfg, a.ray_start, a.ray_end)))
    ref = dict(fx['rendering_kwargs'])
    # the package's one documented difference (nsr/triplane.py OBJAVERSE_RENDERING_KWARGS): the per-sample tensors are opt-in
    assert ref.pop('return_sampling_details_flag') is True and rk.pop('return_sampling_details_flag') is False
    assert rk == ref


def test_shapenet_class_refuses_unknown_cfg_and_other_engines():
    with pytest.raises(SystemExit) as e:
        validate(_args(_COMMON.replace('shapenet_tuneray_aug_resolution_64_64_nearestSR', 'shapenet_tuneray_aug_resolution_64')))
    assert 'shapenet_tuneray_aug_resolution_64' in str(e.value)
    with pytest.raises(SystemExit):
        validate(create_argparser(True).parse_known_args(["--ae_classname", CLASS])[0])       # the DiT / sgm path
    # without the class, --cfg is not read (today's Objaverse-decoder path is unchanged)
    a = _args(_COMMON.replace('--ae_classname ' + CLASS, '').replace('shapenet_tuneray_aug_resolution_64_64_nearestSR', 'no_such_cfg'))
    assert validate(a) == 'gd'


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


def test_new_symbols_are_exported():
    from ln3diff_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libln3d_hip.so not built')
    L = _lib.lib()
    for s in ('ln3d_triplane_axis_attention', 'ln3d_sr_unpatchify', 'ln3d_resize_bilinear_cl', 'ln3d_resize_add_lrelu', 'ln3d_rollout_means',
              'ln3d_im2col3x3_rollout'):
        assert hasattr(L, s)
