#!/usr/bin/env python
"""VAE reconstruction entry point - what the reference's released launcher shell_scripts/final_release/inference/vae_xl_reconstruction.sh
does with the `mv-sd-dit-dynaInp-trilatent` VAE (DiT2-L/2 decoder): posed views -> tri-plane latent -> renders, saving
<logdir>/<ins>/latent.npy (eval_novelview_loop(save_latent=True), nsr/train_nv_util.py:1176-1213).  Body: ln3diff_amd.pipeline.reconstruct.

The encoder input is a tensor file (torch.save / .npy) of shape [B*F, 10, 256, 256], F = --num_frames consecutive views per object.
Assembling it from a dataset is not done here; per view the channels are (datasets/g_buffer_objaverse.py:613-638):
    0-2  RGB normalised to [-1, 1]
    3-8  Pluecker rays of the view's camera: o x d (3-5), then d (6-8) - ln3diff_amd.ops.plucker_rays(c, 256) computes them
         from [V, 25] cameras
    9    depth normalised to [-1, 1]
with the cameras canonicalised the way the reference's dataset does.  Render cameras: --cams, a [V, 25] tensor file (cam2world 4x4 +
normalised intrinsics 3x3), or --n_views orbit cameras.

    python scripts/vae_reconstruction.py --input views.pt --rec_model_path vae.pt --logdir ./logs/rec [--cams cams.pt] [--export_mesh]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _load_tensor(path):
    return torch.from_numpy(np.load(path)) if str(path).endswith('.npy') else torch.load(path, map_location='cpu', weights_only=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--input', required=True, help='encoder input [B*F, 10, 256, 256] (.pt / .npy)')
    ap.add_argument('--rec_model_path', default='', help='VAE checkpoint holding encoder and decoder; empty: synthetic weights (testing)')
    ap.add_argument('--logdir', default='./logs/vae_reconstruction')
    ap.add_argument('--num_frames', type=int, default=6)
    ap.add_argument('--dino_version', default='mv-sd-dit-dynaInp-trilatent')
    ap.add_argument('--arch_dit_decoder', default='DiT2-L/2')
    ap.add_argument('--image_size', type=int, default=128, help='render resolution')
    ap.add_argument('--cams', default='', help='[V, 25] render cameras (.pt / .npy); empty: --n_views orbit cameras')
    ap.add_argument('--n_views', type=int, default=24)
    ap.add_argument('--ins', nargs='*', default=None, help='instance names (one per object); default 0, 1, ...')
    ap.add_argument('--mode', action='store_true', help='use the posterior mode instead of a sample')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--export_mesh', action='store_true')
    ap.add_argument('--mesh_size', type=int, default=192)
    ap.add_argument('--mesh_thres', type=float, default=10.0)
    args = ap.parse_args()

    from ln3diff_amd.checkpoint import load_checkpoint
    from ln3diff_amd.dit.dit_decoder import DiT2_models
    from ln3diff_amd.entry import _save_ppm
    from ln3diff_amd.nsr.script_util import AE
    from ln3diff_amd.nsr.triplane import Triplane
    from ln3diff_amd.pipeline import reconstruct
    from ln3diff_amd.synth import fill_module_random_, orbit_cameras
    from ln3diff_amd.vit.mv_encoder import create_encoder
    from ln3diff_amd.vit.vit_triplane import RodinSR_256_fusionv6_ConvQuant_liteSR_dinoInit3DAttn_SD_B_3L_C_withrollout_withSD_D_ditDecoder as Dec

    dev = torch.device('cuda')
    torch.manual_seed(args.seed)
    enc = create_encoder(dino_version=args.dino_version, num_frames=args.num_frames)
    width = {'DiT2-B/2': 768, 'DiT2-L/2': 1024, 'DiT2-XL/2': 1152}[args.arch_dit_decoder]
    vit = DiT2_models[args.arch_dit_decoder](input_size=16, num_classes=0, learn_sigma=False, in_channels=width, mixed_prediction=False,
                                             context_dim=None, roll_out=True, plane_n=3)
    dec = Dec(vit_decoder=vit, triplane_decoder=Triplane(img_resolution=args.image_size), cls_token=False, vae_p=2, ldm_z_channels=4,
              ldm_embed_dim=4)
    enc, dec = enc.to(dev), dec.to(dev)
    if args.rec_model_path:
        rep = load_checkpoint(args.rec_model_path, decoder=dec, encoder=enc)
        print(f'[vae_reconstruction] loaded {args.rec_model_path}: {rep}')
    else:
        print('[vae_reconstruction] WARNING: no --rec_model_path: SYNTHETIC random weights')
        fill_module_random_(enc, 0, dev)
        fill_module_random_(dec, 1, dev)
    ae = AE(enc, dec, args.image_size, dino_version=args.dino_version)

    img = _load_tensor(args.input).float().to(dev)
    cams = (_load_tensor(args.cams).float() if args.cams else orbit_cameras(args.n_views)).to(dev)
    latent_dir = os.path.join(args.logdir, 'latents')
    out = reconstruct(ae, img, cams, latent_dir=latent_dir, ins_names=args.ins, sample_posterior=not args.mode,
                      export_mesh=args.export_mesh, mesh_size=args.mesh_size, mesh_thres=args.mesh_thres,
                      mesh_path=os.path.join(args.logdir, 'mesh_{}.obj') if args.export_mesh else None)
    frames = out['image_raw'].cpu().numpy()
    names = args.ins or [str(b) for b in range(frames.shape[0])]
    for b, name in enumerate(names):
        d = os.path.join(args.logdir, 'frames', name)
        os.makedirs(d, exist_ok=True)
        for v in range(frames.shape[1]):
            _save_ppm(os.path.join(d, f'{v:03d}.ppm'), frames[b, v])
    print(f'[vae_reconstruction] {len(names)} object(s): latents under {latent_dir}, {frames.shape[1]} frames each under '
          f'{os.path.join(args.logdir, "frames")}')


if __name__ == '__main__':
    main()
