#!/usr/bin/env python
"""fp32 vs fp16 tri-plane texels on one box (GPU only; measurement tool, not product): the ray-marcher with the Objaverse preset on 40
orbit cameras at 256^2 and at 512^2, one generic preset (ShapeNet: 64 + 64 samples, numeric ray limits, render_generic_kernel) at 128^2,
ln3d_query_points on a 192^3 grid, and the converter itself - one process, the two precisions alternating over the rounds on the same
256 x 256 tri-plane (the fp16 planes are the converter's output of the fp32 ones), with socket power / shader clock sampled by
tools/power_sampler.py in a side process.  `python tools/plane_precision_bench.py [rounds] [out_dir]` (defaults 3, bench_out/plane_fp16);
prints a markdown table, writes out_dir/plane_fp16_bench.json and the power trace out_dir/plane_fp16_power.csv
(profiles/plane_fp16_bench.md).  PLANE_BENCH_PROFILE=1: one short pass without the power sampler (for a kernel trace or counter run)."""
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ln3diff_amd import ops  # noqa: E402
from ln3diff_amd.nsr.triplane import Triplane, OBJAVERSE_RENDERING_KWARGS  # noqa: E402
from ln3diff_amd.synth import orbit_cameras  # noqa: E402

PROFILE = os.environ.get('PLANE_BENCH_PROFILE') == '1'
ROUNDS = 1 if PROFILE else (int(sys.argv[1]) if len(sys.argv) > 1 else 3)
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'bench_out', 'plane_fp16')
os.makedirs(OUT, exist_ok=True)
REPS = 1 if PROFILE else 3
csv = os.path.join(OUT, 'plane_fp16_power.csv')
stop = csv + '.stop'
sampler = None
if not PROFILE:
    for f in (csv, stop):
        if os.path.exists(f):
            os.remove(f)
    sampler = subprocess.Popen([sys.executable, os.path.join(ROOT, 'tools', 'power_sampler.py'), csv, '20', stop],
                               stderr=open(os.path.join(OUT, 'plane_fp16_power_sampler.err'), 'w'))
    time.sleep(2.0)
dev = torch.device('cuda:0')
g = torch.Generator(device=dev).manual_seed(0)
SHAPENET = dict(OBJAVERSE_RENDERING_KWARGS, ray_start=0.6, ray_end=1.8, box_warp=1.0, sampler_bbox_min=-0.5, sampler_bbox_max=0.5)
tps = {'objaverse': Triplane(img_resolution=256).to(dev), 'shapenet': Triplane(img_resolution=128, rendering_kwargs=SHAPENET).to(dev)}
for tp in tps.values():
    tp.decoder.net[2].bias.data[0] += 4.0
nchw = torch.randn(1, 96, 256, 256, device=dev, generator=g) * 4             # the decoders' plane tensor: 25 MB in f32
planes = {'fp32': tps['objaverse'].to_channel_last(nchw)}
planes['fp16'] = tps['objaverse'].set_plane_precision('fp16').to_channel_last(nchw)
tps['objaverse'].set_plane_precision('fp32')
assert planes['fp16'].dtype == torch.float16 and torch.equal(planes['fp16'], planes['fp32'].clamp(-65504, 65504).half())
phases, ms = [], {}


def timed(name, prec, fn, per):
    """REPS back-to-back calls between two events, the best of 3 such groups; ms per `per` units"""
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(REPS):
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / REPS)
    ms.setdefault(name, {}).setdefault(prec, []).append(best / per)
    phases.append(dict(name=f'{name} ({prec})', t0=t0, t1=time.time(), ms=round(best / per, 4)))


def render_case(kind, res, V):
    tp = tps[kind]
    cams = orbit_cameras(V).to(dev)
    idx = torch.zeros(V, dtype=torch.int32, device=dev)
    j = torch.rand(V, res * res, 64, device=dev, generator=g)
    u = torch.rand(V * res * res, 64, device=dev, generator=g)
    return lambda p: tp(c=cams, planes_channel_last=p, plane_index=idx, neural_rendering_resolution=res, jitter=j, u_fine=u, views_per_call=1)


G = 192
ax = torch.linspace(-0.45, 0.45, G, device=dev)
pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), dim=-1).reshape(-1, 3).contiguous()
out16 = torch.empty(1, 3, 256, 256, 32, dtype=torch.float16, device=dev)
cl16 = torch.empty_like(out16)
CASES = [('render 256^2, Objaverse 64+64, ms/view of 40', render_case('objaverse', 256, 40), 40),
         ('render 512^2, Objaverse 64+64, ms/view of 40', render_case('objaverse', 512, 40), 40),
         ('render 128^2, ShapeNet preset (generic kernel), ms/view of 8', render_case('shapenet', 128, 8), 8),
         ('query_points 192^3 grid, ms', lambda p: tps['objaverse'].query_points(p[0], pts), 1)]
if PROFILE:                                          # one resolution per kernel name: the per-kernel sums stay readable
    CASES = [c for c in CASES if '512^2' not in c[0]]
for r in range(ROUNDS):
    for name, fn, per in CASES:
        for prec in ('fp32', 'fp16') if r % 2 == 0 else ('fp16', 'fp32'):
            timed(name, prec, lambda: fn(planes[prec]), per)
    timed('converter NCHW f32 -> channel-last f16, one 256^2 tri-plane, ms', 'fp16', lambda: ops.planes_to_channel_last_f16(nchw, out16, 1, 32, 256, 256), 1)
    timed('converter channel-last f32 -> f16, one 256^2 tri-plane, ms', 'fp16', lambda: ops.planes_f32_to_f16(planes['fp32'], cl16), 1)
    timed('converter NCHW f32 -> channel-last f32 (existing), ms', 'fp32', lambda: tps['objaverse'].to_channel_last(nchw), 1)
o32, o16 = CASES[0][1](planes['fp32']), CASES[0][1](planes['fp16'])
rel = {k: float((o16[k] - o32[k]).norm() / o32[k].norm()) for k in ('image_raw', 'image_depth', 'weights_samples')}
rows, src = [], '?'
if sampler is not None:
    time.sleep(1.0)
    open(stop, 'w').close()
    sampler.wait(timeout=20)
    cols = ['t', 'power_w', 'cap_w', 'sclk_mhz', 'sclk_min', 'sclk_max', 'hotspot_c', 'mem_c', 'uclk_mhz', 'throttle', 'gfx_busy', 'energy']
    if os.path.exists(csv):
        for line in open(csv):
            if line.startswith('# source='):
                src = line.strip()[9:]
            if line.startswith('#') or line.startswith('t,'):
                continue
            rows.append([float(a) for a in line.strip().split(',')])
    ix = {c: i for i, c in enumerate(cols)}

    def stat(ph, c):
        v = [r_[ix[c]] for r_ in rows if ph['t0'] <= r_[0] <= ph['t1'] and r_[ix[c]] == r_[ix[c]]]
        return (sum(v) / len(v), min(v), len(v)) if v else (float('nan'), float('nan'), 0)

    print('power source: %s, %d samples' % (src, len(rows)))
    print('| phase | ms | power W mean | sclk MHz mean / min | samples |')
    print('|---|---|---|---|---|')
    for ph in phases:
        pw, sc = stat(ph, 'power_w'), stat(ph, 'sclk_mhz')
        ph.update(power_w=round(pw[0], 1), sclk_mhz=round(sc[0], 0), sclk_min=round(sc[1], 0), samples=pw[2])
        print('| %s | %.4f | %.0f | %.0f / %.0f | %d |' % (ph['name'], ph['ms'], pw[0], sc[0], sc[1], pw[2]))
print('\n| case | fp32 (rounds) | fp16 (rounds) | fp32 / fp16, medians |')
print('|---|---|---|---|')
med = lambda v: sorted(v)[len(v) // 2]
summary = {}
for name, d in ms.items():
    a, b = d.get('fp32'), d.get('fp16')
    ratio = med(a) / med(b) if a and b else float('nan')
    summary[name] = dict(fp32=a, fp16=b, ratio=ratio)
    print('| %s | %s | %s | %s |' % (name, [round(v, 4) for v in a] if a else '', [round(v, 4) for v in b] if b else '', '%.3f' % ratio if a and b else ''))
print('\n256^2 x 40 views, fp16 planes vs fp32 planes, rel-L2: ' + ', '.join('%s %.3e' % kv for kv in rel.items()))
json.dump(dict(source=src, phases=phases, summary=summary, picture_rel_l2=rel, rounds=ROUNDS), open(os.path.join(OUT, 'plane_fp16_bench.json'), 'w'), indent=1)
