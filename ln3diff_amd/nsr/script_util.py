"""`AE` - the reconstruction-model wrapper the reference's drivers talk to (nsr/script_util.py:25-377): everything goes through
`forward(img, c, latent, behaviour, ...)` "for DDP use".  The decoder behaviours that `render_video_given_triplane` /
`eval_i23d_and_export` use run on the HIP decoder.  The encoder behaviours need the released multi-view encoder
(vit/mv_encoder.py, dino_version 'mv-sd-dit-dynaInp-trilatent'); `AE(None, decoder, ...)` - the sampling configuration - raises
NotImplementedError for them.

    enc                        : img [B*F, 10, S, S] -> pooled encoder output [B, 24, S/8, S/8]
    encoder_vae                : enc + decoder.vae_reparameterization(., True) (the frame mean is fused into the posterior kernel)
    dec / dec_wo_triplane      : encoder output -> decoder.vit_decode (sampled posterior) [-> triplane_decode]
    enc_dec / enc_dec_wo_triplane : the two above on img
    (encoder behaviours accept `eps` [B, 4, 3, H*W]: the posterior noise instead of the CPU-generator draw)

    decode_after_vae_no_render : latent dict -> + 'latent_after_vit' [B,96,128,128] (+ 'planes_channel_last' for the renderer)
    triplane_dec               : tri-planes (dict or tensor) + c [V,25] -> Triplane.forward dict (image_raw, image_depth, ...)
    decode_after_vae           : the two above in one call
    triplane_decode_grid       : tri-planes + grid_size -> {'sigma': [B,G,G,G,1], 'rgb': [B,G,G,G,3]}
    triplane_renderer          : tri-planes + coordinates / directions -> decoder output at points (forward_points)
    vit_postprocess_triplane_dec, get_rendering_kwargs
"""
import torch
import torch.nn as nn

_ENCODER_BEHAVIOURS = ('enc_dec', 'enc', 'dec', 'dec_wo_triplane', 'enc_dec_wo_triplane', 'encoder_vae')


class AE(nn.Module):
    def __init__(self, encoder, decoder, img_size, encoder_cls_token=False, decoder_cls_token=False, preprocess=None, use_clip=False,
                 dino_version='sd_dit', clip_dtype=None, no_dim_up_mlp=True, dim_up_mlp_as_func=False, uvit_skip_encoder=False,
                 confnet=None):
        super().__init__()
        if encoder is not None:
            from ..vit.mv_encoder import RELEASED_DINO_VERSION, MVEncoderGSDynamicInp
            if dino_version != RELEASED_DINO_VERSION or not isinstance(encoder, MVEncoderGSDynamicInp):
                raise NotImplementedError(f"AE: the encoder behaviours are built for the released multi-view encoder only "
                                          f"(MVEncoderGSDynamicInp, dino_version={RELEASED_DINO_VERSION!r}); got dino_version={dino_version!r}")
        self.encoder = encoder
        self.decoder = decoder
        self.img_size = img_size
        self.encoder_cls_token, self.decoder_cls_token = encoder_cls_token, decoder_cls_token
        self.use_clip, self.dino_version, self.confnet = use_clip, dino_version, confnet
        self.preprocess = preprocess
        self.dim_up_mlp = None
        self.dim_up_mlp_as_func = dim_up_mlp_as_func

    def decode_after_vae_no_render(self, ret_dict, img_size=None):
        if img_size is None:
            img_size = self.img_size
        assert self.dim_up_mlp is None
        latent = self.decoder.vit_decode_backbone(ret_dict, img_size)
        return self.decoder.vit_decode_postprocess(latent, ret_dict)

    def decode_after_vae(self, ret_dict, c, img_size=None, return_raw_only=False, **kwargs):
        ret_dict = self.decode_after_vae_no_render(ret_dict, img_size)
        return self.decoder.triplane_decode(ret_dict, c, return_raw_only=return_raw_only, **kwargs)

    def encode(self, img):
        return self.encoder(img)

    def encoder_vae(self, img, eps=None):
        """encode + vae_reparameterization(., True), with the per-frame encoder output handed to the posterior kernel (which takes the
        frame mean itself: the same bits as pooling first)."""
        h = self.encoder.forward_frames(img)
        return self.decoder.vae_reparameterization(h, True, eps=eps, num_frames=self.encoder.num_frames)

    def decode_wo_triplane(self, latent, c=None, img_size=None, eps=None):
        return self.decoder.vit_decode(latent, img_size or self.img_size, eps=eps)

    def decode(self, latent, c, img_size=None, return_raw_only=False, eps=None, **kwargs):
        ret = self.decode_wo_triplane(latent, c, img_size, eps=eps)
        return self.decoder.triplane_decode(ret, c, return_raw_only=return_raw_only, **kwargs)

    @torch.no_grad()
    def forward(self, img=None, c=None, latent=None, behaviour='enc_dec', coordinates=None, directions=None, return_raw_only=False,
                *args, **kwargs):
        if behaviour in _ENCODER_BEHAVIOURS:
            if self.encoder is None:
                raise NotImplementedError(f"AE behaviour '{behaviour}' needs the VAE encoder: this AE was built without one "
                                          f"(pass the released MVEncoderGSDynamicInp, vit/mv_encoder.py)")
            eps = kwargs.pop('eps', None)
            if behaviour == 'enc':
                return self.encode(img)
            if behaviour == 'encoder_vae':
                return self.encoder_vae(img, eps)
            if behaviour == 'enc_dec':           # the reference: encode, vit_decode (sampled posterior), triplane_decode
                h = self.encoder.forward_frames(img)
                ret = self.decoder.vit_decode(h, self.img_size, eps=eps, num_frames=self.encoder.num_frames)
                return self.decoder.triplane_decode(ret, c, return_raw_only=return_raw_only, **kwargs)
            if behaviour == 'enc_dec_wo_triplane':
                h = self.encoder.forward_frames(img)
                return self.decoder.vit_decode(h, self.img_size, eps=eps, num_frames=self.encoder.num_frames)
            assert latent is not None
            if behaviour == 'dec':
                return self.decode(latent, c, self.img_size, return_raw_only=return_raw_only, eps=eps, **kwargs)
            return self.decode_wo_triplane(latent, c, self.img_size, eps=eps)          # dec_wo_triplane
        if behaviour == 'decode_after_vae_no_render':
            return self.decode_after_vae_no_render(latent, self.img_size)
        if behaviour == 'decode_after_vae':
            return self.decode_after_vae(latent, c, self.img_size, return_raw_only, **kwargs)
        if behaviour == 'triplane_dec':
            assert latent is not None
            return self.decoder.triplane_decode(latent, c, return_raw_only=return_raw_only, **kwargs)
        if behaviour == 'triplane_decode_grid':
            assert latent is not None
            return self.decoder.triplane_decode_grid(latent, **kwargs)
        if behaviour == 'vit_postprocess_triplane_dec':
            assert latent is not None
            return self.decoder.triplane_decode(self.decoder.vit_decode_postprocess(latent, {}), c)
        if behaviour == 'triplane_renderer':
            assert latent is not None
            return self.decoder.triplane_renderer(latent, coordinates, directions)
        if behaviour == 'get_rendering_kwargs':
            return self.decoder.triplane_decoder.rendering_kwargs
        raise ValueError(f"unknown AE behaviour '{behaviour}'")


class AE_with_Diffusion(nn.Module):          # nsr/script_util.py:386-410 (container used by the joint trainers)
    def __init__(self, auto_encoder, denoise_model):
        super().__init__()
        self.auto_encoder = auto_encoder
        self.denoise_model = denoise_model

    def forward(self, img, c, behaviour='enc_dec', latent=None, *args, **kwargs):
        return self.auto_encoder(img, c, behaviour=behaviour, latent=latent, *args, **kwargs)
