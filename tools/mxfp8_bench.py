#!/usr/bin/env python
"""bf16 vs MX-FP8 on one box (GPU only; measurement tool, not product): the three GEMMs that DiT_TriLatent.set_matmul_precision('mxfp8')
moves to MXFP8, isolated at the configs[1] shapes (DiT-L/2, network batch 16 = 12288 tokens), then the configs[1] denoise loop (B = 8,
CFG 6.5 -> network batch 16, EulerEDM) in both precisions, alternating, with socket power / shader clock sampled by tools/power_sampler.py
in a side process.  `python tools/mxfp8_bench.py [denoise_steps] [rounds] [out_dir]` (defaults 50, 2, bench_out/mxfp8); prints a markdown
table, writes out_dir/mxfp8_bench.json and the power trace out_dir/mxfp8_power.csv (profiles/mxfp8_bench.md)."""
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ln3diff_amd import ops  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'bench_out', 'mxfp8')
os.makedirs(OUT, exist_ok=True)
SEC = float(os.environ.get('MXFP8_BENCH_SEC', '2'))
csv = os.path.join(OUT, 'mxfp8_power.csv')
stop = csv + '.stop'
for f in (csv, stop):
    if os.path.exists(f):
        os.remove(f)
sampler = subprocess.Popen([sys.executable, os.path.join(ROOT, 'tools', 'power_sampler.py'), csv, '20', stop],
                           stderr=open(os.path.join(OUT, 'mxfp8_power_sampler.err'), 'w'))
dev = torch.device('cuda:0')
phases = []


def loop(name, fn, flops):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, n = time.time(), 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    while time.time() - t0 < SEC:
        for _ in range(50):
            fn()
        n += 50
        torch.cuda.synchronize()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / n
    phases.append(dict(name=name, t0=t0, t1=time.time(), launches=n, avg_us=round(us, 2), tflops=round(flops / us / 1e6, 1)))
    time.sleep(0.5)


time.sleep(2.0)
M, D, F, H, N = 16 * 768, 1024, 4096, 16, 768
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(M, D, device=dev, generator=g)
f1in = torch.randn(M, F, device=dev, generator=g)
wq = torch.randn(3 * D, D, device=dev, generator=g) * 0.03
w1 = torch.randn(F, D, device=dev, generator=g) * 0.03
w2 = torch.randn(D, F, device=dev, generator=g) * 0.02
b3, b1, bD = (torch.randn(n, device=dev, generator=g) * 0.02 for n in (3 * D, F, D))
gate = torch.randn(16, 6 * D, device=dev, generator=g) * 0.1
res = torch.zeros(M, D, device=dev)
q = torch.zeros(16, H, N, 64, dtype=torch.bfloat16, device=dev)
k, vt = torch.zeros_like(q), torch.zeros(16, H, 64, N, dtype=torch.bfloat16, device=dev)
heads = dict(M=M, tokens=N, tok_pad=N, heads=H, head_dim=64, transpose_mask=0b100, head_dim_pad=64)
xb, f1b, wqb, w1b, w2b = (t.bfloat16() for t in (x, f1in, wq, w1, w2))
xm, f1m, wqm, w1m, w2m = (ops.quantize_mx(t) for t in (x, f1in, wq, w1, w2))
yb = torch.empty(M, F, dtype=torch.bfloat16, device=dev)
ym = ops.MX.empty(M, F, dev)
for prec in ('bf16', 'mxfp8'):
    bf = prec == 'bf16'
    loop(f'QKV + head split ({prec})', (lambda: ops.gemm(xb, wqb, b3, ops.EPI_HEADS, q, k, vt, **heads)) if bf else
         (lambda: ops.gemm_mx(xm, wqm, b3, ops.EPI_HEADS, q, k, vt, **heads)), 2.0 * M * 3 * D * D)
    loop(f'fc1 + GELU ({prec}{"" if bf else ", MXFP8 out"})', (lambda: ops.gemm(xb, w1b, b1, ops.EPI_GELU_ERF, yb)) if bf else
         (lambda: ops.gemm_mx(xm, w1m, b1, ops.EPI_GELU_ERF, ym.q, out_scale=ym.s)), 2.0 * M * F * D)
    loop(f'fc2 + gate/residual ({prec})', (lambda: ops.gemm(f1b, w2b, bD, ops.EPI_GATE_RES, res, gate=gate, gate_rows=N, gate_ld=6 * D)) if bf else
         (lambda: ops.gemm_mx(f1m, w2m, bD, ops.EPI_GATE_RES, res, gate=gate, gate_rows=N, gate_ld=6 * D)), 2.0 * M * D * F)
del x, f1in, xb, f1b, xm, f1m, yb, ym, res
torch.cuda.empty_cache()

# configs[1]'s denoise loop: DiT-L/2 (random weights, bench.py's fill), B = 8 -> network batch 16, EulerEDM + CFG 6.5
from ln3diff_amd.dit.dit_trilatent import DiT_models  # noqa: E402
from ln3diff_amd.dit.dit_models_xformers import TextCondDiTBlock  # noqa: E402
from ln3diff_amd.synth import fill_module_random_  # noqa: E402
from ln3diff_amd.sgm.sampling import EulerEDMSampler, DiscreteDenoiser, VanillaCFG  # noqa: E402
with dev:
    dit = DiT_models['DiT-L/2'](input_size=32, num_classes=0, learn_sigma=False, in_channels=4, context_dim=768, roll_out=True,
                                vit_blk=TextCondDiTBlock)
dit = dit.to(dev)
fill_module_random_(dit, 0, dev)
B = 8
z = torch.randn(B, 12, 32, 32, device=dev, generator=g)
cond = {'crossattn': torch.randn(B, 77, 768, device=dev, generator=g)}
uc = {'crossattn': torch.zeros_like(cond['crossattn'])}
sampler_ = EulerEDMSampler(num_steps=STEPS, guider=VanillaCFG(6.5))
lat = {}
for prec in ('bf16', 'mxfp8'):                     # warm-up (packing) of both
    dit.set_matmul_precision(prec)
    lat[prec] = sampler_(DiscreteDenoiser().bind(dit), z.clone(), cond, uc)
torch.cuda.synchronize()
step_ms = {'bf16': [], 'mxfp8': []}
for r in range(ROUNDS):
    for prec in ('bf16', 'mxfp8') if r % 2 == 0 else ('mxfp8', 'bf16'):
        dit.set_matmul_precision(prec)
        sampler_(DiscreteDenoiser().bind(dit), z.clone(), cond, uc)      # repack + warm
        torch.cuda.synchronize()
        t0 = time.time()
        sampler_(DiscreteDenoiser().bind(dit), z.clone(), cond, uc)
        torch.cuda.synchronize()
        t1 = time.time()
        ms = (t1 - t0) * 1e3 / (STEPS - 1)                  # EulerEDM: num_steps sigmas -> num_steps - 1 network evaluations
        step_ms[prec].append(ms)
        phases.append(dict(name=f'configs[1] denoise loop ({prec}), round {r}', t0=t0, t1=t1, launches=STEPS - 1, avg_us=round(ms * 1e3, 1)))
        time.sleep(0.5)
rel = float((lat['mxfp8'] - lat['bf16']).norm() / lat['bf16'].norm())
time.sleep(1.0)
open(stop, 'w').close()
sampler.wait(timeout=20)

rows, src = [], '?'
cols = ['t', 'power_w', 'cap_w', 'sclk_mhz', 'sclk_min', 'sclk_max', 'hotspot_c', 'mem_c', 'uclk_mhz', 'throttle', 'gfx_busy', 'energy']
if os.path.exists(csv):
    for line in open(csv):
        if line.startswith('# source='):
            src = line.strip()[9:]
        if line.startswith('#') or line.startswith('t,'):
            continue
        rows.append([float(a) for a in line.strip().split(',')])
ix = {c: i for i, c in enumerate(cols)}


def stat(ph, c, skip=0.2):
    v = [r[ix[c]] for r in rows if ph['t0'] + skip <= r[0] <= ph['t1'] and r[ix[c]] == r[ix[c]]]
    return (sum(v) / len(v), min(v), len(v)) if v else (float('nan'), float('nan'), 0)


print('power source: %s, %d samples' % (src, len(rows)))
print('| phase | launches | avg us | TFLOP/s | power W mean | cap W | sclk MHz mean / min | samples |')
print('|---|---|---|---|---|---|---|---|')
for ph in phases:
    pw, cp, sc = stat(ph, 'power_w'), stat(ph, 'cap_w'), stat(ph, 'sclk_mhz')
    ph.update(power_w=round(pw[0], 1), cap_w=round(cp[0], 1), sclk_mhz=round(sc[0], 0), sclk_min=round(sc[1], 0), samples=pw[2])
    print('| %s | %d | %s | %s | %.0f | %.0f | %.0f / %.0f | %d |' % (ph['name'], ph['launches'], ph['avg_us'], ph.get('tflops', ''), pw[0], cp[0],
                                                                    sc[0], sc[1], pw[2]))
med = {p: sorted(v)[len(v) // 2] for p, v in step_ms.items()}
print('\ndenoise step (one CFG network evaluation, network batch 16), ms: bf16 %s, mxfp8 %s -> speed-up %.3fx' % (
    [round(v, 2) for v in step_ms['bf16']], [round(v, 2) for v in step_ms['mxfp8']], med['bf16'] / med['mxfp8']))
print('final latent after %d steps, mxfp8 vs bf16 rel-L2: %.3e' % (STEPS, rel))
json.dump(dict(source=src, phases=phases, step_ms=step_ms, speedup=med['bf16'] / med['mxfp8'], latent_rel_l2=rel, steps=STEPS),
          open(os.path.join(OUT, 'mxfp8_bench.json'), 'w'), indent=1)
