"""Host cost of marshalling one call into libln3d_hip.so, without a GPU: three entry points called with a NULL first buffer, so each
returns LN3D_ERR_BAD_ARG before anything is launched.  Arguments are built the way ln3diff_amd/ops.py builds them: plain values where
_lib declares argtypes (PROTOTYPES), ctypes wrappers per argument where it does not (the binding before the table), so the same file
measures either commit.  gemm_plan and attention_plan go further: valid buffers (never dereferenced) and a request that the entry point
refuses with LN3D_ERR_UNSUPPORTED only after its whole kernel choice has run (a qk_norm on 32-wide heads at DiT-L/2's QKV shape; 96-wide
heads), which is the host cost of ln3d_gemm_bf16 / ln3d_attention_bf16 up to the launch.  LN3D_LIB selects another build.
usage: python tools/abi_call_cost.py [calls] [repeats]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ln3diff_amd import _lib  # noqa: E402

calls = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
typed = hasattr(_lib, 'PROTOTYPES')
if os.environ.get('LN3D_LIB'):
    _lib.LIB_PATH = os.path.abspath(os.environ['LN3D_LIB'])
L = _lib.lib()
ADDR = 0x10000                                                                                   # never dereferenced
gemm_args = _lib.GemmArgs(X=None, ldx=1024, W=ADDR, ldw=1024, M=12288, N=3072, K=1024, epilogue=_lib.EPI_HEADS, out0=ADDR, out1=ADDR, out2=ADDR,
                          ldo=3072, tokens=768, tok_pad=768, heads=16, head_dim=64, transpose_mask=4)
plan_args = _lib.GemmArgs(X=ADDR, ldx=1024, W=ADDR, ldw=1024, M=12288, N=3072, K=1024, epilogue=_lib.EPI_HEADS, out0=ADDR, out1=ADDR, out2=ADDR,
                          ldo=3072, tokens=768, tok_pad=768, heads=96, head_dim=32, transpose_mask=4, head_norm0=ADDR)
attn_args = _lib.AttnArgs(Q=ADDR, K=ADDR, Vt=ADDR, O=ADDR, B=16, H=16, Nq=768, Nq_pad=768, Nk=768, Nk_pad=768, Dh=96, ldo=1536, scale=0.1)
if typed:
    def ddim_step():
        return L.ln3d_ddim_step(None, ADDR, ADDR, ADDR, 3.0, 1.1, 0.4, 0.9, 0.2, 0.0, True, 49152, 0)

    def final_layer():
        return L.ln3d_final_layer(None, ADDR, ADDR, 6144, ADDR, ADDR, ADDR, ADDR, ADDR, 16, 4, 32, 2, 1024, 0)

    def gemm():
        return L.ln3d_gemm_bf16(gemm_args, 0)

    def gemm_plan():
        return L.ln3d_gemm_bf16(plan_args, 0)

    def attention_plan():
        return L.ln3d_attention_bf16(attn_args, 0)
else:
    P, I64, F = C.c_void_p, C.c_int64, C.c_float

    def ddim_step():
        return L.ln3d_ddim_step(None, P(ADDR), P(ADDR), P(ADDR), F(3.0), F(1.1), F(0.4), F(0.9), F(0.2), F(0.0), int(True), I64(49152), P(0))

    def final_layer():
        return L.ln3d_final_layer(None, P(ADDR), P(ADDR), I64(6144), P(ADDR), P(ADDR), P(ADDR), P(ADDR), P(ADDR), 16, 4, 32, 2, 1024, P(0))

    def gemm():
        return L.ln3d_gemm_bf16(C.byref(gemm_args), P(0))

    def gemm_plan():
        return L.ln3d_gemm_bf16(C.byref(plan_args), P(0))

    def attention_plan():
        return L.ln3d_attention_bf16(C.byref(attn_args), P(0))


print("binding with %s; %d calls, %d repeats; microseconds per call" % ("argtypes" if typed else "per-argument ctypes wrappers", calls, repeats))
for fn, refusal in ((ddim_step, -1), (final_layer, -1), (gemm, -1), (gemm_plan, -3), (attention_plan, -3)):
    assert fn() == refusal, fn.__name__                                                         # LN3D_ERR_*: nothing was launched
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        us.append((time.perf_counter() - t0) / calls * 1e6)
    print("%-14s best %.3f  repeats %s" % (fn.__name__, min(us), ' '.join('%.3f' % u for u in us)))
