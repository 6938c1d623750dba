#!/usr/bin/env python
"""Bitwise A/B listing for changes to the memory-bound glue kernels of ln3diff_amd/csrc that serve several entry points, or that one
entry point mirrors from another: the 3x3 im2col (ln3d_im2col3x3 / _strided / _pad01), norm + modulate (ln3d_norm_modulate / _mx), the plane layout
(ln3d_planes_to_channel_last / _f16) and the roll-out means (ln3d_rollout_means / _bf16).  Seeded inputs go through ln3diff_amd.ops and
every output buffer - its guard tail included - is printed as one sha256 line.  Each tree loads its own libln3d_hip.so, so run it once
per tree, each run its own process, and diff the listings:

    python tools/glue_ab.py [--tree OTHER_CHECKOUT] > listing.txt

Only `ops` is used, so the same file runs against an older checkout (--tree)."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='checkout to import ln3diff_amd from')
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ln3diff_amd  # noqa: E402
from ln3diff_amd import ops  # noqa: E402
assert os.path.abspath(ln3diff_amd.__file__).startswith(ROOT + os.sep), (ln3diff_amd.__file__, ROOT)

DEV = 'cuda'
BF = torch.bfloat16
TAIL = 64                                   # guard elements behind every output, part of its digest


def gen(*key):
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], 'little'))


def out(case, name, t):
    h = hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]
    print(f'{case} {name} {str(t.dtype)[6:]}[{t.numel()}] {h}')


def guarded(n, dtype):
    """n elements + TAIL guard elements of a fixed pattern, on the device"""
    fill = 0x5a if dtype == torch.uint8 else 7.0
    return torch.full((n + TAIL,), fill, dtype=dtype, device=DEV)


# ---------------------------------------------------------------- im2col: the shapes of the tests and one workload shape per front
def im2col():
    plain = [(2, H, W, C, up, K) for H, W in ((1, 1), (5, 7), (8, 3)) for C, K in ((8, 80), (16, 160), (64, 576)) for up in (1, 2)]
    plain += [(6, 64, 64, 64, 2, 576), (6, 128, 128, 64, 1, 576)]                      # the Objaverse decoder's two largest
    for N, H, W, C, up, K in plain:
        x = torch.randn(N, H, W, C, generator=gen('i2c', N, H, W, C)).to(BF).to(DEV)
        col = guarded(N * H * up * W * up * K, BF)
        ops.im2col3x3(x, col, N, H, W, C, up, K)
        out(f'im2col3x3/N{N}_H{H}_W{W}_C{C}_up{up}_K{K}', 'col', col)
    strided = [(N, H, W, C, s, 9 * C + e) for s in (1, 2) for H, W in ((1, 1), (7, 8), (8, 7), (32, 32)) for C in (8, 16, 320) for e in (0, 24)
               for N in (1, 3)]
    strided += [(2, 32, 96, 128, 2, 1152)]                                             # the U-Net's Downsample
    for N, H, W, C, s, K in strided:
        x = torch.randn(N, H, W, C, generator=gen('i2s', N, H, W, C)).to(BF).to(DEV)
        col = guarded(N * ((H - 1) // s + 1) * ((W - 1) // s + 1) * K, BF)
        ops.im2col3x3_strided(x, col, N, H, W, C, s, K)
        out(f'im2col3x3_strided/N{N}_H{H}_W{W}_C{C}_s{s}_K{K}', 'col', col)
    pad01 = [(N, H, W, C, 9 * C + e) for H, W in ((2, 2), (7, 8), (8, 7), (32, 32)) for C, e in ((8, 0), (64, 16)) for N in (1, 3)]
    pad01 += [(6, 64, 64, 64, 576)]                                                    # the multi-view encoder's first Downsample
    for N, H, W, C, K in pad01:
        x = torch.randn(N, H, W, C, generator=gen('i2p', N, H, W, C)).to(BF).to(DEV)
        col = guarded(N * ((H - 2) // 2 + 1) * ((W - 2) // 2 + 1) * K, BF)
        ops.im2col3x3_pad01(x, col, N, H, W, C, K)
        out(f'im2col3x3_pad01/N{N}_H{H}_W{W}_C{C}_K{K}', 'col', col)


# ---------------------------------------------------------------- norm + modulate, bf16 output
def norm_modulate():
    S, rows_in = 3, 11
    rows = S * rows_in
    for D, kind in ((512, 0), (1024, 1), (1536, 0), (1536, 1), (128, 1), (768, 0), (1152, 0), (1152, 1), (1280, 0), (1280, 1)):
        for mod in (False, True):
            for form in ('plain', 'tables', 'remap'):
                if form == 'tables' and not mod:
                    continue
                g = gen('nm', D, kind, mod, form)
                x = (torch.randn(rows, D, generator=g) + 0.3 + 5.0 * torch.randn(rows, 1, generator=g)).to(DEV)
                kw = {}
                if kind == 1:
                    kw['weight'] = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV)
                if mod:
                    buf = (torch.randn(S, 3 * D, generator=g) * 0.5).to(DEV)
                    kw.update(shift=buf[:, :D], scale=buf[:, D:2 * D], mod_rows=rows_in, mod_ld=3 * D)
                if form == 'tables':
                    kw.update(shift_table=(0.1 * torch.randn(D, generator=g)).to(DEV), scale_table=(0.1 * torch.randn(D, generator=g)).to(DEV))
                rows_out = 14 if form == 'remap' else rows_in
                if form == 'remap':
                    kw.update(rows_in=rows_in, rows_out=rows_out)
                y = guarded(S * rows_out * D, BF)
                ops.norm_modulate(x, y, rows, D, kind=kind, eps=1e-6, **kw)
                out(f'norm_modulate/D{D}_kind{kind}_mod{int(mod)}_{form}', 'y', y)


# ---------------------------------------------------------------- norm + modulate, MXFP8 output
def norm_modulate_mx():
    widths = [128, 512, 640, 1024, 1152, 1280, 1536]
    row_sets = [(1, 1), (3, 1), (5, 2), (1000, 250)]
    cases = []
    for i, D in enumerate(widths):                 # the sparse cross of tests/test_mx_elements_gpu.py
        for kind in (0, 1):
            cases.append((D, kind, row_sets[(i + 2 * kind) % 4], bool((i + kind) & 1), bool(((i >> 1) + kind) & 1), False))
    cases += [(D, kind, (8, 2), True, True, True) for D in (512, 1152, 1536) for kind in (0, 1)]          # the special rows
    for D, kind, (rows, mod_rows), weighted, mod, special in cases:
        g = gen('nmx', D, kind, rows, weighted, mod, special)
        x = torch.randn(rows, D, generator=g) * torch.exp2(torch.randint(-12, 12, (rows, 1), generator=g).float()) + 0.1
        if special:
            x[1, 5] = float('inf'); x[2, D - 1] = float('-inf'); x[3, 77] = float('nan')
            x[4] *= 3.0e19                                                                               # squares overflow f32
            x[5, 0] = float('nan'); x[5, 64] = float('inf')
        kw = {}
        if weighted:
            kw['weight'] = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV)
        if mod:
            md = (torch.randn((rows + mod_rows - 1) // mod_rows, 6 * D, generator=g) * 0.5).to(DEV)
            kw.update(shift=md[:, D:2 * D], scale=md[:, 4 * D:5 * D], mod_rows=mod_rows, mod_ld=6 * D)
        y = ops.MX(guarded(rows * D, torch.uint8), guarded(rows * (D // 32), torch.uint8))
        ops.norm_modulate_mx(x.to(DEV), y, rows, D, kind=kind, eps=1e-6, **kw)
        case = f'norm_modulate_mx/D{D}_kind{kind}_rows{rows}_w{int(weighted)}_mod{int(mod)}_special{int(special)}'
        out(case, 'q', y.q)
        out(case, 's', y.s)


# ---------------------------------------------------------------- plane layout, f32 and binary16 texels
def planes():
    for NP, H, W in ((2, 7, 7), (1, 33, 9), (4, 256, 256)):
        g = gen('pl', NP, H, W)
        src = torch.randn(NP, 96, H, W, generator=g)
        dst = guarded(NP * 96 * H * W, torch.float32)
        ops.planes_to_channel_last(src.to(DEV), dst, NP, 32, H, W)
        out(f'planes_to_channel_last/NP{NP}_H{H}_W{W}', 'dst', dst)
        src = src * 3.0e4                                                    # a good part beyond +-65504
        flat = src.view(-1)
        flat[3] = float('nan'); flat[flat.numel() // 2] = float('inf'); flat[-5] = float('-inf'); flat[11] = 65520.0; flat[12] = -65519.9
        dst = guarded(NP * 96 * H * W, torch.float16)
        ops.planes_to_channel_last_f16(src.to(DEV), dst, NP, 32, H, W)
        out(f'planes_to_channel_last_f16/NP{NP}_H{H}_W{W}', 'dst', dst)


# ---------------------------------------------------------------- roll-out means of f32 and bf16 planes
def rollout_means():
    for H, W, C in ((9, 13, 300), (256, 256, 128)):
        for dtype in (torch.float32, BF):
            x = torch.randn(3, H, W, C, generator=gen('rm', H, W, C))
            x[..., 1::2] += 1000.0
            rowm, colm = guarded(3 * H * C, torch.float32), guarded(3 * W * C, torch.float32)
            ops.rollout_means(x.to(dtype).to(DEV), rowm[:3 * H * C], colm[:3 * W * C], 3, H, W, C)
            case = f'rollout_means/{str(dtype)[6:]}_H{H}_W{W}_C{C}'
            out(case, 'rowmean', rowm)
            out(case, 'colmean', colm)


if __name__ == '__main__':
    im2col()
    norm_modulate()
    norm_modulate_mx()
    planes()
    rollout_means()
    torch.cuda.synchronize()
